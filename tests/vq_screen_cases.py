"""Adversarial inputs of the VQ nearest-code search for any (N, C, E): the case list of
test_kernels_gpu.py::test_vq_screened_argmin_equals_the_exact_scan, generated from the shape instead of fixed row numbers.
Shared by tests/test_vq_screen_widths_cpu.py and tests/test_vq_screen_widths_gpu.py."""
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FINITE_CASES = ['gauss', 'duplicates', 'clustered', 'tiny', 'huge', 'rows_on_codes', 'mixed_scale']
CASES = FINITE_CASES + ['nan_row']


def table_widths():
    """The widths csrc/vq_screen_widths.h instantiates the screened search for."""
    with open(os.path.join(ROOT, 'world_modelz_amd', 'csrc', 'vq_screen_widths.h')) as f:
        line = next(ln for ln in f if ln.startswith('#define WMZ_VQ_SCREEN_WIDTHS'))
    return [int(w) for w in re.findall(r'X\((\d+)\)', line)]


def applies(case, C):
    return C >= 3 or case != 'duplicates'


def make_case(case, N, C, E, seed=11):
    """(x [N, E], codebook [C, E]) fp32 on the CPU."""
    g = torch.Generator().manual_seed(seed + 1000 * E + C)
    x, cb = torch.randn(N, E, generator=g), torch.randn(C, E, generator=g)
    if case == 'duplicates':                     # three equal codes (first, middle, last) and 64 rows next to them
        assert C >= 3
        cb[C // 2] = cb[0]
        cb[C - 1] = cb[0]
        x[:64] = cb[0] + 1e-3 * torch.randn(64, E, generator=g)
    elif case == 'clustered':                    # clusters of ~32 codes 1e-4 apart: every row's best codes are near ties
        centers = torch.randn(max(1, C // 32), E, generator=g)
        cb = centers[torch.arange(C) % centers.shape[0]] + 1e-4 * torch.randn(C, E, generator=g)
    elif case == 'tiny':
        x, cb = x * 1e-3, cb * 1e-3
    elif case == 'huge':
        x, cb = x * 300.0, cb * 300.0
    elif case == 'rows_on_codes':
        n = min(N, C)
        x[:n] = cb[:n]
    elif case == 'nan_row':
        x[min(5, N - 1), min(3, E - 1)] = float('nan')
    elif case == 'mixed_scale':                  # one huge code sets emax: the bound widens for every row
        cb[min(9, C - 1)] = cb[min(9, C - 1)] * 1e3
    else:
        assert case == 'gauss', case
    return x, cb
