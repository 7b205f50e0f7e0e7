"""The attention backward kernels (csrc/attn_bwd.hip, csrc/attn_bwd_row16.hip) element by element against a dense fp64 reference,
on every kernel instantiation their dispatch can launch (tests/attn_bounds.py: the cases, the route each takes, the bound;
tests/test_attn_bounds_cpu.py holds that helper to account without a GPU).  For every case: dq, dk, dv inside the per-element
bound and the Frobenius bars of tests/test_backward_gpu.py, written into sentinel frames (a head's padded lanes must not write
past the row), bit-equal on a second call.  One case per route family also as the q | k | v column thirds of one buffer, and
support probes -- where a gradient may be non-zero at all -- on the general, 16-wide and 8-wide routes.

out and lse come from the fp64 oracle (out rounded to the kernel's type, lse to fp32), not from the forward kernel: the
reference uses the same values, so forward error is no part of a bound.  The forward -> backward hand-over stays with
tests/test_backward_gpu.py and tests/test_attn_32_wide_gpu.py."""
import contextlib

import pytest
import torch

import attn_bounds as ab
import gemm_bounds as gb

pytestmark = pytest.mark.gpu

IDS = [c.id for c in ab.CASES]
NORM_BAR = {ab.F32: 2e-5, ab.BF16: 2e-2}          # tests/test_backward_gpu.py


@pytest.fixture(scope='module')
def wmz():
    assert torch.cuda.is_available()
    from world_modelz_amd import _lib, ops
    return dict(lib=_lib, ops=ops)


def run_framed(L, c, x):
    """wmz_local3d_attn_bwd on the inputs x of case c, dq and dk|dv written into sentinel frames (row strides I + 16 and 2I + 16,
    8 sentinel columns on either side, rows after), the [2, tokens, heads] workspace between sentinels -> dq, dk, dv on the CPU."""
    B, S, H, W = c.shape
    I, M = c.heads * c.dh, B * S * H * W
    q, k, v, do, out, lse = (t.cuda().contiguous() for t in (x.q, x.k, x.v, x.do, x.out, x.lse))
    assert lse.dtype == torch.float32 and lse.shape == (M, c.heads)
    fq, dq, mq = gb.framed(M, I, c.dtype, 'cuda', ld=I + 16)
    fkv, dkv, mkv = gb.framed(M, 2 * I, c.dtype, 'cuda', ld=2 * I + 16)
    fws, ws, mws = gb.framed_flat((2, M, c.heads), torch.float32, 'cuda')
    dk, dv = dkv[:, :I], dkv[:, I:]
    L.call('wmz_local3d_attn_bwd', L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(out), L.ptr(lse), L.ptr(do), L.ptr(dq), L.ptr(dk), L.ptr(dv),
           L.ptr(ws), B, S, H, W, c.heads, c.dh, int(c.ext[0]), int(c.ext[1]), int(c.ext[2]), I, I, I, I, I, I + 16, 2 * I + 16,
           2 * I + 16, L.dtype_code(c.dtype), L.stream())
    torch.cuda.synchronize()
    for buf, mask in ((fq, mq), (fkv, mkv), (fws, mws)):
        gb.assert_untouched(buf, mask)
    return dq.cpu(), dk.cpu(), dv.cpu()


def check_all(tag, c, x, got):
    """gemm_bounds.check on dq, dk, dv: every element, and the Frobenius bar.  The bar is a RELATIVE norm: it is left out for a
    tensor whose reference is zero up to its own error bound (|ref| < |e_in| in norm -- dq and dk where every token sees itself
    only: out = v makes dS = P (dO.v - dO.out) cancel completely, what is left is the rounding of out).  The element-wise check
    holds there as everywhere."""
    worst = []
    for name, g in zip(('dq', 'dk', 'dv'), got):
        ref, e_in = x.ref[name], x.ref['e_' + name]
        cancelled = float(ref.norm()) < float(e_in.norm())
        assert not cancelled or (c.ext == (0, 0, 0) and name != 'dv'), (tag, name)
        worst.append(gb.check(f'{tag} {name}', g, ref, e_in, norm_tol=None if cancelled else NORM_BAR[c.dtype]))
    return worst


@pytest.mark.parametrize('cid', IDS)
def test_attention_backward_inside_the_elementwise_bound(wmz, cid):
    c, x = ab.CASE[cid], ab.case_inputs(cid)
    got = run_framed(wmz['lib'], c, x)
    diff = [float(((gb.f64(g) - x.ref[n]).abs() / ab.tolerance(x.ref[n], x.ref['e_' + n], g.dtype)).max())
            for n, g in zip(('dq', 'dk', 'dv'), got)]
    print(f'[{cid}] {" | ".join(ab.case_routes(c))}: worst ratio dq {diff[0]:.3f} dk {diff[1]:.3f} dv {diff[2]:.3f}')
    check_all(cid, c, x, got)
    again = run_framed(wmz['lib'], c, x)
    for name, a, b in zip(('dq', 'dk', 'dv'), got, again):
        assert torch.equal(a, b), f'{name}: a second call is not bit-equal'


@contextlib.contextmanager
def recorded_args(L, name):
    """The argument tuples of every call of entry point `name` inside the block."""
    seen, orig = [], L.call

    def call(n, *a):
        if n == name:
            seen.append(a)
        return orig(n, *a)
    L.call = call
    try:
        yield seen
    finally:
        L.call = orig


@pytest.mark.parametrize('cid', ab.THIRDS)
def test_attention_backward_column_thirds_bit_equal(wmz, cid):
    """q | k | v as the column thirds of one [.., 3I] buffer and dq | dk | dv written into the thirds of another (config 5's fused
    to_qkv): row stride 3I on six operands, bit-equal to the contiguous call and inside the bound.  On 16 x 16 planes this is the
    dk|dv plane kernel compiled for two different visitor row strides."""
    L, ops = wmz['lib'], wmz['ops']
    c, x = ab.CASE[cid], ab.case_inputs(cid)
    B, S, H, W = c.shape
    I = c.heads * c.dh
    out, lse, do = x.out.cuda(), x.lse.cuda(), x.do.cuda()
    dq, dkv = ops.local3d_attention_bwd(x.q.cuda(), x.k.cuda(), x.v.cuda(), out, lse, do, c.ext, c.heads)
    qkv = torch.cat([x.q, x.k, x.v], -1).cuda()
    dqkv = torch.full((B, S, H, W, 3 * I), float('nan'), dtype=c.dtype, device='cuda')
    with recorded_args(L, 'wmz_local3d_attn_bwd') as seen:
        ops.local3d_attention_bwd(qkv[..., :I], qkv[..., I:2 * I], qkv[..., 2 * I:], out, lse, do, c.ext, c.heads, dqkv=dqkv)
    assert len(seen) == 1 and tuple(seen[0][19:27]) == (3 * I, 3 * I, 3 * I, I, I, 3 * I, 3 * I, 3 * I), seen[0][19:27]
    torch.cuda.synchronize()
    assert torch.equal(dqkv[..., :I], dq) and torch.equal(dqkv[..., I:], dkv)
    got = tuple(dqkv[..., j * I:(j + 1) * I].reshape(-1, I).cpu() for j in range(3))
    w = check_all(cid, c, x, got)
    print(f'[{cid}] thirds: {" | ".join(ab.case_routes(c, thirds=True))}: worst ratio dq {w[0]:.3f} dk {w[1]:.3f} dv {w[2]:.3f}')


@pytest.mark.parametrize('cid', list(ab.PROBES))
def test_attention_backward_support_probes(wmz, cid):
    """Where a gradient may be non-zero.  dO non-zero at ONE query: the dk and dv rows are exactly zero outside that query's window
    and non-zero inside it.  K non-zero at ONE key: the dq rows are exactly zero for queries that do not see the key and non-zero
    for those that do.  Each probe element-wise inside the bound as well (rows that must be zero have a zero tolerance)."""
    L = wmz['lib']
    c, x = ab.CASE[cid], ab.case_inputs(cid)
    B, S, H, W = c.shape
    N = S * H * W
    mask = ab.window_mask(S, H, W, c.ext)

    def live_rows(g):
        return (g != 0).any(-1).reshape(B, N)

    for s, h, w in ab.PROBES[cid]:
        tok = (s * H + h) * W + w
        expect = torch.zeros(B, N, dtype=torch.bool)
        expect[0] = mask[tok]                                                   # symmetric: sees / is seen by
        one_do = torch.zeros_like(x.do)
        one_do[0, s, h, w] = x.do[0, s, h, w]
        y = ab.types.SimpleNamespace(q=x.q, k=x.k, v=x.v, do=one_do, out=x.out, lse=x.lse,
                                     ref=ab.bwd_ref(x.q, x.k, x.v, one_do, x.out, x.lse, c.ext, c.heads, ab.case_family(c)))
        got = run_framed(L, c, y)
        check_all(f'{cid} dO at {(s, h, w)}', c, y, got)
        for name, g in zip(('dk', 'dv'), got[1:]):
            assert torch.equal(live_rows(g), expect), (name, (s, h, w), (live_rows(g) != expect).nonzero()[:4])
        one_k = torch.zeros_like(x.k)
        one_k[0, s, h, w] = x.k[0, s, h, w]
        y = ab.make_inputs(c, x.q, one_k, x.v, x.do)
        got = run_framed(L, c, y)
        check_all(f'{cid} K at {(s, h, w)}', c, y, got)
        assert torch.equal(live_rows(got[0]), expect), ('dq', (s, h, w), (live_rows(got[0]) != expect).nonzero()[:4])
