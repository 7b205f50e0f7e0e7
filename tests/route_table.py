"""The denoiser's inference and training dispatch written out from config.py's documented rules -- the tables that
tests/test_route_matrix_gpu.py runs on the GPU and tests/test_parallel_cpu.py pins against fused.inference_route /
fused.training_route on the host.  They are deliberately NOT derived from fused.supported / chain_supported / chain_pays /
half_attention_ok: a change of those gates has to change these tables too."""
import torch

MODES = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'precise': torch.float16}

# (dim, heads, dim_head, mlp_dim) at depth 2
WIDTHS = [
    (256, 1, 128, 256),     # the default: fused
    (256, 2, 64, 256),      # fused
    (256, 4, 32, 256),      # fused
    (256, 8, 16, 256),      # fused in bf16; no half attention for dim_head 16
    (96, 1, 128, 256),      # published: chain
    (128, 3, 64, 256),      # the reference's test() geometry: chain
    (160, 1, 128, 256),     # off the chain table: op by op
    (64, 8, 64, 96),        # the module's own default heads: op by op
    (64, 1, 64, 96),        # quirk Q6: to_out is Identity -- op by op
    (64, 3, 20, 96),        # heads off the 8-element granule (zero-padded): op by op
]

# planes (H, W); S = 3, B = 2 in the GPU matrix
PLANES = [(16, 16), (6, 16), (1, 16), (8, 8), (2, 8), (7, 8), (12, 12), (5, 7), (4, 20)]
# ... and of the training matrix: 7 x 8 is 336 tokens, no multiple of 32
TRAIN_PLANES = [(16, 16), (7, 8), (12, 12)]

# (dim, dim_head * heads, mlp_dim) of the fused per-token kernels (csrc/layer_fused.hip) ...
FUSED_WIDTHS = {(256, 128, 256)}
# ... and of the chain kernels (csrc/chain_widths.h)
CHAIN_WIDTHS = {(96, 128, 256), (384, 128, 512), (128, 192, 256), (128, 128, 256), (128, 128, 512), (192, 128, 512),
                (256, 128, 512), (256, 128, 1024), (256, 256, 256), (256, 256, 512), (256, 256, 1024), (512, 128, 1024)}

# the half attention unit: heads of these widths, planes 16 wide or 8 wide with an even row count
HALF_DIM_HEADS = (32, 64, 128)


def half_plane(H, W):
    return W == 16 or (W == 8 and H % 2 == 0)


def is_identity(dim, heads, dh):
    return heads == 1 and dh == dim                 # quirk Q6: no to_out projection, which no fused kernel holds


def expected_route(widths, mode, H, W, chain_policy='always'):
    """'fused' | 'chain' | 'ops' for an inference forward of the model `widths` in `mode` on H x W planes.  chain_policy is
    config.chain_policy ('always' / 'never'; bf16 only -- the precise mode takes the half chain kernels whenever it can)."""
    dim, heads, dh, mlp = widths
    if mode == 'fp32' or is_identity(dim, heads, dh):
        return 'ops'
    if mode == 'precise' and (dh not in HALF_DIM_HEADS or not half_plane(H, W)):
        return 'ops'                                # the fp32 route: never bf16, never an error
    key = (dim, heads * dh, mlp)
    if key in FUSED_WIDTHS:
        return 'fused'
    if key in CHAIN_WIDTHS and (mode == 'precise' or chain_policy == 'always'):
        return 'chain'
    return 'ops'


def expected_training_route(widths, mode, ntok, fused_backward=True, chain_policy='always'):
    """(forward, backward kernels) of a DenoiserTrainer step of the model `widths` in `mode` on ntok tokens, the fused training
    switch on: forward 'fused' | 'chain' | 'ops', backward kernels True where that forward's own backward kernels run (else the
    op-by-op block backward).  Training has no half kernels: the precise mode trains on the fp32 route, op by op.  The fused
    backward kernels work on whole 32-token tiles; the chain kernels train in bf16 under chain_policy 'always' (the trainer's
    step; a module called outside a trainer holds no chain packs and trains op by op)."""
    dim, heads, dh, mlp = widths
    if mode != 'bf16' or is_identity(dim, heads, dh):
        return 'ops', False
    key = (dim, heads * dh, mlp)
    if key in FUSED_WIDTHS:
        return 'fused', fused_backward and ntok % 32 == 0
    if key in CHAIN_WIDTHS and chain_policy == 'always':
        return 'chain', fused_backward
    return 'ops', False


# entry points that identify a route
FUSED_ENTRIES = ('wmz_layer_fused_fwd_planes', 'wmz_embed_qkv_fused_fwd_planes')
CHAIN_ENTRIES = ('wmz_layer_chain_fwd_planes',)


def is_fused_or_chain(name):
    return 'layer_fused' in name or 'layer_chain' in name or 'embed_qkv_fused' in name


# the backward kernels of each training family
TRAIN_BWD_ENTRIES = {'fused': ('wmz_ff_fused_bwd', 'wmz_qkv_fused_bwd'), 'chain': ('wmz_chain_ff_bwd', 'wmz_chain_qkv_bwd')}
