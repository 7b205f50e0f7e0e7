"""The screened nearest-code search (csrc/vq_screen.hip) at every width of csrc/vq_screen_widths.h and any codebook size: the route
ops.vq_argmin takes, bit identity with the full scan in the pinned fp32 order and with the oracle, that both of its halves (the
screening's decision, the exact re-check) really run, the quantiser module on top of it, and a captured call."""
import copy

import pytest
import torch

from conftest import recorded_calls
from oracle import vq as ovq
from vq_screen_cases import CASES, applies, make_case, table_widths

pytestmark = pytest.mark.gpu

WIDTHS = table_widths()
N = 333                                     # three workgroups of 128 rows, the last one ragged


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'gpu tests need a ROCm device'
    from world_modelz_amd import ops as _ops
    return _ops


def flag_count(ops, device):
    torch.cuda.synchronize()
    return int(ops._vq_screen_ws[device][4:8].view(torch.int32).item())       # workspace header: flag count at byte 4


def test_route_is_the_screened_search_exactly_at_the_table_widths():
    from world_modelz_amd._lib import lib
    need = lib().wmz_vq_argmin_screened_workspace_bytes
    assert WIDTHS == [16, 32, 64, 128, 256]
    for E in WIDTHS:
        assert need(N, 100, E) > 0, E
    assert need(N, 1, 64) > 0 and need(N, 1000, 64) > 0
    for E in (8, 24, 40, 512):
        assert need(N, 100, E) == 0, E
    assert need(0, 100, 64) == 0 and need(N, 0, 64) == 0


@pytest.mark.parametrize('C', [1, 33, 64, 100, 257, 576])
@pytest.mark.parametrize('E', WIDTHS)
def test_screened_equals_the_exact_scan_and_the_oracle(ops, E, C):
    """indices and minimum distances, bit for bit, ties to the lowest index, on every adversarial case"""
    for case in CASES:
        if not applies(case, C):
            continue
        x, cb = make_case(case, N, C, E)
        xd, cbd = x.cuda(), cb.cuda()
        with recorded_calls() as seen:
            idx_s, d_s = ops.vq_argmin(xd, cbd, need_dist=True)
        assert seen == ['wmz_vq_argmin_screened'], (case, seen)
        idx_e, d_e = ops.vq_argmin(xd, cbd, need_dist=True, exact_scan=True)
        assert torch.equal(idx_s, idx_e), case
        assert torch.equal(torch.nan_to_num(d_s, nan=-1.0), torch.nan_to_num(d_e, nan=-1.0)), case
        if case != 'nan_row' and N * C * E <= 5e7:
            ref = ovq.distances(x, cb[None])[:, 0]
            assert torch.equal(idx_s.cpu(), ref.argmin(-1)) and torch.equal(d_s.cpu(), ref.min(-1).values), case


@pytest.mark.parametrize('E', WIDTHS)
def test_the_recheck_really_runs(ops, E):
    """three identical codes and 64 rows next to them: no bound can tell them apart, every one of those rows is re-scanned"""
    x, cb = make_case('duplicates', N, 100, E)
    xd, cbd = x.cuda(), cb.cuda()
    idx = ops.vq_argmin(xd, cbd)
    nflag = flag_count(ops, xd.device)
    print(f'[vq screened] E={E}: {nflag} of {N} rows re-scanned with duplicated codes')
    assert nflag >= 64
    assert torch.equal(idx, ops.vq_argmin(xd, cbd, exact_scan=True))


@pytest.mark.parametrize('E', WIDTHS)
def test_the_screening_really_decides(ops, E):
    """Gaussian data, N = 4096, C = 256: at most a tenth of the rows go to the re-check (a cap against flagging everything, not
    a speed figure: the share computed in exact arithmetic under the bound is below 2 % at every width)."""
    g = torch.Generator().manual_seed(E)
    x, cb = torch.randn(4096, E, generator=g).cuda(), torch.randn(256, E, generator=g).cuda()
    idx = ops.vq_argmin(x, cb)
    nflag = flag_count(ops, x.device)
    print(f'[vq screened] E={E}: {nflag} of 4096 rows re-scanned ({100.0 * nflag / 4096:.2f} %)')
    assert nflag <= 4096 // 10
    assert torch.equal(idx, ops.vq_argmin(x, cb, exact_scan=True))


class _ExactScanOps:
    """world_modelz_amd.ops with the nearest-code search forced to the full scan"""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        return getattr(self._real, name)

    def vq_argmin(self, x, codebook, need_dist=False, exact_scan=False):
        return self._real.vq_argmin(x, codebook, need_dist=need_dist, exact_scan=True)


@pytest.mark.parametrize('E,C,n_lat', [(32, 100, 2), (128, 257, 1), (256, 64, 1)])
def test_quantiser_module_on_the_screened_route(ops, monkeypatch, E, C, n_lat):
    from world_modelz_amd import vq as vqmod
    torch.manual_seed(3)
    m = vqmod.VectorQuantizerEMA(E, C, num_latents=n_lat).cuda()
    m_exact = copy.deepcopy(m)
    # (rows on a grid of 1/64: the EMA statistics' row sums are exact in fp32 whatever order their atomics arrive in, so equal
    #  indices give equal buffers bit for bit)
    x = (torch.randn(N, n_lat * E) * 64).round() / 64
    xd = x.cuda()
    with recorded_calls() as seen:
        idx = m.encode(xd)
    assert seen.count('wmz_vq_argmin_screened') == n_lat and 'wmz_vq_argmin' not in seen    # (the latent views take the new route)
    assert torch.equal(idx.cpu(), ovq.encode(x, m.embedding.cpu()))
    m.train()
    m_exact.train()
    m(xd)
    with monkeypatch.context() as mp:
        mp.setattr(vqmod, 'ops', _ExactScanOps(ops))
        with recorded_calls() as seen:
            m_exact(xd)
    assert 'wmz_vq_argmin_screened' not in seen and seen.count('wmz_vq_argmin') == n_lat
    for name in ('embedding', 'cluster_size', 'activation_count'):
        assert torch.equal(getattr(m, name), getattr(m_exact, name)), name


def test_captured_call_replays(ops):
    """(N = 333, C = 100, E = 128) captured after one eager call (the workspace exists); one stream, no parallel branches"""
    g = torch.Generator().manual_seed(5)
    cb = torch.randn(100, 128, generator=g).cuda()
    xs = [torch.randn(N, 128, generator=g).cuda() for _ in range(3)]
    static_x = xs[0].clone()
    ops.vq_argmin(static_x, cb, need_dist=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        idx, dmin = ops.vq_argmin(static_x, cb, need_dist=True)
    for x in xs[1:]:
        static_x.copy_(x)
        graph.replay()
        idx_e, d_e = ops.vq_argmin(x, cb, need_dist=True, exact_scan=True)
        assert torch.equal(idx, idx_e) and torch.equal(dmin, d_e)
