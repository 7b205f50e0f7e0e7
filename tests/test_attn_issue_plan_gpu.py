"""The headline attention launch (csrc/attn_fwd_row16_infer.hip, <3, 3>: bf16, 16x16 planes, dim_head 128, window (3, 3, 3)) under
the row map and the issue plan of csrc/attn_slab_walk.h: which wave owns a query row and which wave requests a DMA piece must not
show in O.  Bit-identity with the run-time kernel is tests/test_attn_infer_unit_gpu.py; here: every output row is written once and
nothing else is, and each query row sees exactly the key rows of its window."""
import pytest
import torch

pytestmark = pytest.mark.gpu

EXT = (3, 3, 3)
H = W = 16
DH = 128
SENTINEL = 0x7FA5            # a bf16 NaN pattern: no output of finite inputs carries it
GUARD = 4 * W * DH           # four plane rows of elements before and behind O


def launch(q, k, v, o):
    """wmz_local3d_attn_fwd_planes over the whole grid into the caller's O."""
    from world_modelz_amd import _lib as L
    B, S = q.shape[:2]
    L.call('wmz_local3d_attn_fwd_planes', L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(o), None, B, S, H, W, 1, DH, EXT[0], EXT[1], EXT[2],
           DH, DH, DH, DH, 0, S, L.dtype_code(q.dtype), L.stream())
    torch.cuda.synchronize()


def qkv(B, S, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, S, H, W, DH, generator=g).bfloat16().cuda() for _ in range(3)]


@pytest.mark.parametrize('B,S', [(1, 1), (2, 5)])
def test_o_is_fully_written_and_framed(B, S):
    """O pre-filled with a NaN pattern between guard rows of the same pattern: afterwards none of it is left inside (a query row
    nobody owns under the permutation) and the guards are untouched (a row written outside the plane)."""
    q, k, v = qkv(B, S, seed=10 * B + S)
    n = B * S * H * W * DH
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.int16, device='cuda')
    o = buf[GUARD:GUARD + n].view(torch.bfloat16).view(B, S, H, W, DH)
    launch(q, k, v, o)
    inside = buf[GUARD:GUARD + n].view(B * S, H, W * DH)
    unwritten = (inside == SENTINEL).any(dim=2).nonzero().tolist()
    assert not unwritten, f'(plane, row) left unwritten: {unwritten[:8]}'
    assert torch.isfinite(o.float()).all()
    assert (buf[:GUARD] == SENTINEL).all() and (buf[GUARD + n:] == SENTINEL).all()
    # a doubled row would also leave another one unwritten; what was written is the run-time kernel's
    from world_modelz_amd import _lib as L
    ref = torch.empty_like(o)
    L.call('wmz_debug_attn_knobs', 0, 1)
    try:
        launch(q, k, v, ref)
    finally:
        L.call('wmz_debug_attn_knobs', 0, 0)
    assert torch.equal(o, ref)


@pytest.fixture(scope='module')
def one_plane():
    q, k, v = qkv(1, 1, seed=77)
    o = torch.empty_like(q)
    launch(q, k, v, o)
    return q, k, v, o


@pytest.mark.parametrize('r', [0, 3, 8, 12, 15])
def test_a_key_row_reaches_exactly_the_query_rows_of_its_window(one_plane, r):
    """S = 1.  Key row r (K and V) replaced: the query rows r - 3 .. r + 3 change, every token of them (each sees at least four
    tokens of the row), and all other rows keep their bits -- each wave's lo / hi after the remap."""
    q, k, v, base = one_plane
    g = torch.Generator().manual_seed(1000 + r)
    k2, v2 = k.clone(), v.clone()
    k2[0, 0, r] = (3 * torch.randn(W, DH, generator=g)).bfloat16().cuda()
    v2[0, 0, r] = (3 * torch.randn(W, DH, generator=g)).bfloat16().cuda()
    o = torch.empty_like(q)
    launch(q, k2, v2, o)
    changed = (o[0, 0].view(torch.int16) != base[0, 0].view(torch.int16)).any(dim=2)        # [query row, token]
    rows_any = changed.any(dim=1).nonzero().flatten().tolist()
    want = list(range(max(0, r - EXT[1]), min(H - 1, r + EXT[1]) + 1))
    assert rows_any == want, (r, rows_any)
    assert changed[want].all(), (r, (~changed[want]).nonzero().tolist()[:8])
