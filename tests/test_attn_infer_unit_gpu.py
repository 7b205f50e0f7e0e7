"""The inference unit of the row16 attention forward (csrc/attn_fwd_row16_infer.hip: bf16, 16x16 planes, dim_head 128, one head, row
strides 128, extents 3,3 or 1,1 in the plane, the slab walk compiled in) against the run-time kernel it replaces, bit for bit.

wmz_debug_attn_knobs(0, 1) keeps the run-time kernel where the unit would run; every case runs once per route on the same inputs.
The launches attn_fwd_impl must NOT hand to the unit (H = 12, two heads, dim_head 64, a row stride of 256, an LSE request) run the
same way: both routes are then the run-time kernel, and the results are checked against the oracle as well."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import attention as oat          # noqa: E402

ORACLE_REL = 3e-3            # the row kernel's bound in tests/test_kernels_gpu.py (P and the output are rounded to bf16)
WINDOWS = [(3, 3, 3), (3, 1, 1)]             # the headline window and the published 7x3x3 one


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@contextlib.contextmanager
def variant(value):
    from world_modelz_amd import _lib as L
    L.call('wmz_debug_attn_knobs', 0, value)
    try:
        yield
    finally:
        L.call('wmz_debug_attn_knobs', 0, 0)


def both_routes(fn):
    """fn() -> tensors, once with the dispatch left alone and once with the run-time kernel kept."""
    with variant(0):
        new = [t.clone() for t in fn()]
    with variant(1):
        old = [t.clone() for t in fn()]
    torch.cuda.synchronize()
    return new, old


def qkv(shape, heads=1, dh=128, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*shape, heads * dh, generator=g).bfloat16() for _ in range(3)]


def fwd(q, k, v, ext, heads=1, need_lse=False):
    from world_modelz_amd import ops
    return both_routes(lambda: [t for t in ops.local3d_attention_fwd(q.cuda(), k.cuda(), v.cuda(), ext, heads, need_lse=need_lse)
                                if t is not None])


def fwd_planes(q, k, v, ext, q0, nq):
    """wmz_local3d_attn_fwd_planes: the query planes [q0, q0 + nq) only, compact output."""
    from world_modelz_amd import _lib as L
    B, S, H, W, I = q.shape
    qd, kd, vd = q.cuda(), k.cuda(), v.cuda()

    def run():
        o = torch.zeros((B, nq, H, W, I), dtype=q.dtype, device='cuda')
        L.call('wmz_local3d_attn_fwd_planes', L.ptr(qd), L.ptr(kd), L.ptr(vd), L.ptr(o), None, B, S, H, W, 1, I, int(ext[0]),
               int(ext[1]), int(ext[2]), I, I, I, I, q0, nq, L.dtype_code(q.dtype), L.stream())
        return [o]
    return both_routes(run)


@pytest.mark.parametrize('ext', WINDOWS)
@pytest.mark.parametrize('S', [1, 2, 4, 7, 8, 9])
def test_full_grid_matches_the_runtime_kernel_bit_for_bit(S, ext):
    """B = 1: fewer planes than the window (1, 2, 4), exactly the window (7), the rotated order's wrap (8, 9)."""
    q, k, v = qkv((1, S, 16, 16), seed=S)
    (new,), (old,) = fwd(q, k, v, ext)
    assert torch.isfinite(new.float()).all()
    assert torch.equal(new, old)


@pytest.mark.parametrize('ext', WINDOWS)
def test_batch_stride_and_a_grid_that_is_no_multiple_of_eight(ext):
    """B = 3, S = 5: 15 workgroups over the 8 XCDs; against the oracle as well (one case per extents pair)."""
    q, k, v = qkv((3, 5, 16, 16), seed=35)
    (new,), (old,) = fwd(q, k, v, ext)
    assert torch.equal(new, old)
    ref = oat.local_attention(k.float(), v.float(), q.float(), ext, 1)
    e = rel(new, ref)
    print(f'[attn infer unit {ext}] out vs oracle {e:.2e}')
    assert e < ORACLE_REL


@pytest.mark.parametrize('ext', WINDOWS)
@pytest.mark.parametrize('q0,nq', [(8, 1), (3, 4)])
def test_trailing_planes_count_the_phase_from_the_clips_end(q0, nq, ext):
    """S = 9, query planes [q0, q0 + nq): equal between the routes, and equal to those planes of the full grid (same visiting order,
    hence the same roundings)."""
    q, k, v = qkv((1, 9, 16, 16), seed=9)
    (new,), (old,) = fwd_planes(q, k, v, ext, q0, nq)
    assert torch.equal(new, old)
    (full,), _ = fwd(q, k, v, ext)
    assert torch.equal(new, full[:, q0:q0 + nq])


@pytest.mark.parametrize('ext', WINDOWS)
def test_rescale_branch_and_an_all_tie_plane(ext):
    """q scaled until the logits of consecutive steps differ by far more than the deferral of 2^8 (the rescale fires again and
    again; exp2 underflows), and, separately, a key plane of equal values (every logit of that plane ties)."""
    q, k, v = qkv((1, 4, 16, 16), seed=4)
    (new,), (old,) = fwd((q.float() * 200).bfloat16(), k, v, ext)
    assert torch.isfinite(new.float()).all()
    assert torch.equal(new, old)
    k2 = k.clone()
    k2[0, 2] = 0.25
    (new,), (old,) = fwd(q, k2, v, ext)
    assert torch.equal(new, old)
    assert rel(new, oat.local_attention(k2.float(), v.float(), q.float(), ext, 1)) < ORACLE_REL


@pytest.mark.parametrize('what', ['H12', 'heads2', 'dh64', 'stride256', 'lse'])
def test_launches_outside_the_unit_keep_the_runtime_kernel(what):
    ext = (3, 3, 3)
    shape, heads, dh = ((1, 3, 12, 16) if what == 'H12' else (1, 3, 16, 16)), (2 if what == 'heads2' else 1), (64 if what == 'dh64' else 128)
    q, k, v = qkv(shape, heads, dh, seed=12)
    if what == 'stride256':                     # k | v the column halves of one buffer
        kv = torch.cat([k, v], dim=-1).cuda()
        kd, vd = kv[..., :128], kv[..., 128:]
    else:
        kd, vd = k, v
    new, old = fwd(q, kd, vd, ext, heads, need_lse=what == 'lse')
    assert len(new) == (2 if what == 'lse' else 1)
    for a, b in zip(new, old):
        assert torch.equal(a, b)
    assert rel(new[0], oat.local_attention(k.float(), v.float(), q.float(), ext, heads)) < ORACLE_REL
