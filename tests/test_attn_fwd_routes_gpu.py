"""The attention forward kernels (csrc/attn_fwd.hip, attn_fwd_row16.hip and its half and 32-wide units, attn_fwd_row16_infer.hip)
element by element against a dense fp64 reference, on every kernel instantiation attn_fwd_impl can launch (tests/attn_fwd_bounds.py:
the cases, the route each takes, the bound; tests/test_attn_fwd_bounds_cpu.py holds that helper to account without a GPU).  For every
case: out and lse inside the per-element bound and out inside the Frobenius bars the suite already holds the forward to, written into
sentinel frames, bit-equal on a second call and with lse = None.  The logit regimes on one case per family; the key-indicator launches,
where every output element is the probability of one query-key pair or an exact zero; the general, planes and window entry points; q |
k | v as column thirds; the logits probe; and the refusal of half operands off the row shapes."""
import pytest
import torch

import attn_fwd_bounds as fb
import gemm_bounds as gb

pytestmark = pytest.mark.gpu

IDS = [c.id for c in fb.CASES]
NORM_BAR = {fb.F32: 1e-5, fb.BF16: 3e-3, fb.F16: 1e-3}        # tests/test_kernels_gpu.py, test_attn_32_wide_gpu.py, test_precise_mode_gpu.py


@pytest.fixture(scope='module')
def L():
    assert torch.cuda.is_available()
    from world_modelz_amd import _lib
    return _lib


def run(L, c, q, k, v, lse=True, probe=False, general=False, flat=False, thirds=False, planes=None):
    """One forward launch of case c on q, k, v -> dict(out [M, I], lse [M, heads] | None, dbg [M, heads, slots] | None) on the CPU.
    out goes into a sentinel frame of row stride I + 16 (flat: row stride I, sentinel rows behind -- the only output the inference
    unit takes), lse and the probe into flat frames; every frame is checked outside what the launch may write.  thirds: q | k | v
    are the column thirds of one buffer (row stride 3 I).  planes = (q0, nq): the query planes [q0, q0 + nq) of a B = 1 case only,
    written where the full grid has them -- every other plane must keep the sentinel.  Entry point: wmz_local3d_attn_fwd, _general,
    _planes, or _window where the time window is one- or two-sided."""
    B, S, H, W = c.shape
    I, M = c.heads * c.dh, B * S * H * W
    eb, ef, eH, eW = c.ext
    if thirds:
        qkv = torch.cat([q, k, v], -1).reshape(M, 3 * I).cuda()
        qd, kd, vd, ld = qkv[:, :I], qkv[:, I:2 * I], qkv[:, 2 * I:], 3 * I
    else:
        qd, kd, vd = (t.reshape(M, I).cuda().contiguous() for t in (q, k, v))
        ld = I
    ldo = I if flat else I + 16
    fo, out, mo = gb.framed(M, I, c.dtype, 'cuda', ld=ldo, left=0 if flat else 8)
    fl, lv, ml = gb.framed_flat((M, c.heads), torch.float32, 'cuda')
    fd, dv, md = gb.framed_flat((M, c.heads, fb.n_slots(c.ext)), torch.float32, 'cuda') if probe else (None, None, None)
    if probe:
        dv.fill_(-1e9)
    q0, nq = (0, S) if planes is None else planes
    if planes is not None:
        assert B == 1 and not probe
        rows = torch.zeros(M, dtype=torch.bool)
        rows[q0 * H * W:(q0 + nq) * H * W] = True
        mo &= torch.cat([rows, torch.zeros(fo.shape[0] - M, dtype=torch.bool)])[:, None]
        ml[64:64 + M * c.heads] = rows.repeat_interleave(c.heads)
    o_ptr = out[q0 * H * W:] if planes is not None else out
    l_ptr = (lv[q0 * H * W:] if planes is not None else lv) if lse else None
    head = (L.ptr(qd), L.ptr(kd), L.ptr(vd), L.ptr(o_ptr), L.ptr(l_ptr))
    dt, st = L.dtype_code(c.dtype), L.stream()
    if eb != ef:
        L.call('wmz_local3d_attn_fwd_window', *head, L.ptr(dv), B, S, H, W, c.heads, c.dh, eb, ef, eH, eW, ld, ld, ld, ldo, q0, nq,
               int(general), dt, st)
    elif planes is not None:
        assert not general
        L.call('wmz_local3d_attn_fwd_planes', *head, B, S, H, W, c.heads, c.dh, eb, eH, eW, ld, ld, ld, ldo, q0, nq, dt, st)
    else:
        L.call('wmz_local3d_attn_fwd_general' if general else 'wmz_local3d_attn_fwd', *head, L.ptr(dv), B, S, H, W, c.heads, c.dh,
               eb, eH, eW, ld, ld, ld, ldo, dt, st)
    torch.cuda.synchronize()
    gb.assert_untouched(fo, mo)
    if lse:
        gb.assert_untouched(fl, ml)
    else:
        gb.assert_untouched(fl, torch.zeros_like(ml))
    if probe:
        gb.assert_untouched(fd, md)
    return dict(out=out.cpu(), lse=lv.cpu() if lse else None, dbg=dv.cpu() if probe else None, rows=None if planes is None else rows)


def check_both(tag, c, ref, got, norm=True):
    w_out = gb.check(f'{tag} out', got['out'], ref.out, ref.e_out, norm_tol=NORM_BAR[c.dtype] if norm else None)
    w_lse = gb.check(f'{tag} lse', got['lse'], ref.lse, ref.e_lse) if got['lse'] is not None else float('nan')
    return w_out, w_lse


def ratios(ref, got):
    """Worst |got - ref| / tol of out and lse, before anything is asserted."""
    r = lambda g, x, e: float(((gb.f64(g) - x).abs() / fb.tolerance(x, e, g.dtype)).nan_to_num(nan=float('inf')).max())      # noqa: E731
    return r(got['out'], ref.out, ref.e_out), r(got['lse'], ref.lse, ref.e_lse)


@pytest.mark.parametrize('cid', IDS)
def test_attention_forward_inside_the_elementwise_bound(L, cid):
    c, x = fb.CASE[cid], fb.case_inputs(cid)
    got = run(L, c, x.q, x.k, x.v)
    print(f'[{cid}] {fb.case_route(c, ld=(c.heads * c.dh,) * 3 + (c.heads * c.dh + 16,))}: worst ratio out %.3f lse %.3f' % ratios(x.ref, got))
    check_both(cid, c, x.ref, got)
    again = run(L, c, x.q, x.k, x.v)
    assert torch.equal(got['out'], again['out']) and torch.equal(got['lse'], again['lse']), 'a second call is not bit-equal'
    bare = run(L, c, x.q, x.k, x.v, lse=False)
    assert torch.equal(got['out'], bare['out']), 'out differs with lse = None'


@pytest.mark.parametrize('cid', fb.INFER_CASES)
def test_inference_unit_inside_the_bound_and_bit_equal_across_the_hand_over(L, cid):
    """Contiguous operands, lse = None: attn_fwd_row16_infer_kernel.  The same launch with lse stays on the run-time kernel; out is
    bit-equal across the hand-over, and inside the bound."""
    c, x = fb.CASE[cid], fb.case_inputs(cid)
    assert fb.case_route(c, lse=False) == fb.INFER.format(c.ext[2]) and 'attn_fwd_row16_kernel<128, Big' in fb.case_route(c, lse=True)
    unit = run(L, c, x.q, x.k, x.v, lse=False, flat=True)
    w = gb.check(f'{cid} out (inference unit)', unit['out'], x.ref.out, x.ref.e_out, norm_tol=NORM_BAR[c.dtype])
    print(f'[{cid}] {fb.case_route(c, lse=False)}: worst ratio out {w:.3f}')
    rt = run(L, c, x.q, x.k, x.v, lse=True, flat=True)
    check_both(cid, c, x.ref, rt)
    assert torch.equal(unit['out'], rt['out'])
    assert torch.equal(unit['out'], run(L, c, x.q, x.k, x.v, lse=False, flat=True)['out'])


@pytest.mark.parametrize('regime', fb.REGIMES[1:])
@pytest.mark.parametrize('cid', fb.REGIME_CASES)
def test_logit_regimes(L, cid, regime):
    c, x = fb.CASE[cid], fb.case_inputs(cid, regime)
    got = run(L, c, x.q, x.k, x.v)
    print(f'[{cid} {regime}] {fb.case_route(c)}: worst ratio out %.3f lse %.3f' % ratios(x.ref, got))
    check_both(f'{cid} {regime}', c, x.ref, got)


@pytest.mark.parametrize('cid', fb.indicator_cases())
def test_key_indicator_launches(L, cid):
    """V_j = e_slot(j): every output element is the probability of ONE query-key pair, or an exact zero where the slot's key is
    outside the window or the grid (e_in = 0 there: the tolerance is TINY, and the stored value must be 0)."""
    c, x, ref = fb.CASE[cid], fb.case_inputs(cid), fb.case_pairs(cid)
    worst = 0.0
    for g in range(fb.n_indicator_launches(c)):
        v = fb.indicator_v(c.shape, c.heads, c.dh, c.ext, g, c.dtype)
        out, e = ref.with_v(v)
        got = run(L, c, x.q, x.k, v, lse=False)['out']
        worst = max(worst, gb.check(f'{cid} indicator launch {g}', got, out, e))
        assert torch.equal(got == 0, out == 0), f'{cid} launch {g}: a pair too many or too few'
    print(f'[{cid}] {fb.case_route(c)}: {fb.n_indicator_launches(c)} indicator launches, worst ratio {worst:.3f}')


@pytest.mark.parametrize('cid', ['w16-h17', 'w16-plane-64', 'w8-t6', 'w8-t16', 'w32-h5-32', 'w32-small', 'w16-asym', 'infer-33'])
def test_general_entry_point_at_row_shapes(L, cid):
    """wmz_local3d_attn_fwd_general (wmz_local3d_attn_fwd_window with general = 1) at a shape of the row routes: the general kernel,
    inside the general bound."""
    c, x = fb.CASE[cid], fb.case_inputs(cid, general=True)
    assert fb.route_family(fb.case_route(c, general=True)) == 'general' and fb.case_family(c) == 'row'
    got = run(L, c, x.q, x.k, x.v, general=True)
    print(f'[{cid}] {fb.case_route(c, general=True)}: worst ratio out %.3f lse %.3f' % ratios(x.ref, got))
    check_both(f'{cid} general', c, x.ref, got)


@pytest.mark.parametrize('cid', fb.PLANES)
def test_query_planes_strictly_inside_the_clip(L, cid):
    """wmz_local3d_attn_fwd_planes / _window with (q0, nq) = (1, 1) and, where the clip has four planes, (1, 2): bit-equal to the
    full-grid call on those planes, the sentinel left on all others (run checks the frames)."""
    c, x = fb.CASE[cid], fb.case_inputs(cid)
    S = c.shape[1]
    flat = cid in fb.INFER_CASES
    for lse in (True, False):
        full = run(L, c, x.q, x.k, x.v, lse=lse, flat=flat)
        for q0, nq in ((1, 1), (1, S - 2)):
            part = run(L, c, x.q, x.k, x.v, lse=lse, flat=flat, planes=(q0, nq))
            rows = part['rows']
            assert torch.equal(part['out'][rows], full['out'][rows])
            assert not lse or torch.equal(part['lse'][rows], full['lse'][rows])
            if lse:
                gb.check(f'{cid} planes out', part['out'][rows], x.ref.out[rows], x.ref.e_out[rows])


@pytest.mark.parametrize('cid', fb.THIRDS)
def test_column_thirds_bit_equal(L, cid):
    c, x = fb.CASE[cid], fb.case_inputs(cid)
    a, b = run(L, c, x.q, x.k, x.v), run(L, c, x.q, x.k, x.v, thirds=True)
    assert torch.equal(a['out'], b['out']) and torch.equal(a['lse'], b['lse'])
    check_both(f'{cid} thirds', c, x.ref, b)


@pytest.mark.parametrize('cid', fb.PROBED)
def test_logits_probe(L, cid):
    """With logits_dbg: out and lse bit-equal to the call without it; the probed logits element-wise inside scale e_s + the
    roundings of sc * G.scale; slots outside the window or the grid keep the caller's -1e9."""
    c, x, ref = fb.CASE[cid], fb.case_inputs(cid), fb.case_pairs(cid)
    plain, probed = run(L, c, x.q, x.k, x.v), run(L, c, x.q, x.k, x.v, probe=True)
    assert torch.equal(plain['out'], probed['out']) and torch.equal(plain['lse'], probed['lse'])
    lg, e = fb.probe_ref(ref, c.shape, c.ext, c.heads)
    w = gb.check(f'{cid} probe', probed['dbg'], lg, e)
    assert torch.equal(probed['dbg'] == -1e9, lg == -1e9)
    print(f'[{cid}] {fb.case_route(c, probe=True)}: probe worst ratio {w:.3f}')


@pytest.mark.parametrize('shape,dh,general', [((1, 2, 5, 7), 64, False), ((1, 2, 7, 8), 64, False), ((1, 2, 16, 16), 40, False),
                                              ((1, 2, 16, 16), 128, True), ((1, 2, 6, 20), 32, False)])
def test_half_off_the_row_shapes_is_refused(L, shape, dh, general):
    """Half operands at a shape off the row routes: WMZ_ERR_UNSUPPORTED, and nothing is launched -- every frame keeps its sentinel."""
    assert fb.fwd_route(shape, dh, fb.F16, general=general) is None
    c = fb._case('half-off', shape, 1, dh, (1, 1, 1), fb.F16)
    q, k, v = fb.make_qkv(c)
    B, S, H, W = shape
    M = B * S * H * W
    fo, out, mo = gb.framed(M, dh, fb.F16, 'cuda', ld=dh + 16)
    fl, lv, ml = gb.framed_flat((M, 1), torch.float32, 'cuda')
    qd, kd, vd = (t.reshape(M, dh).cuda() for t in (q, k, v))
    with pytest.raises(L.WmzError, match=r'code 3'):
        L.call('wmz_local3d_attn_fwd_general' if general else 'wmz_local3d_attn_fwd', L.ptr(qd), L.ptr(kd), L.ptr(vd), L.ptr(out),
               L.ptr(lv), None, B, S, H, W, 1, dh, 1, 1, 1, dh, dh, dh, dh + 16, L.dtype_code(fb.F16), L.stream())
    torch.cuda.synchronize()
    gb.assert_untouched(fo, torch.zeros_like(mo))
    gb.assert_untouched(fl, torch.zeros_like(ml))
