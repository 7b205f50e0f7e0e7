"""The screened nearest-code search at every width of csrc/vq_screen_widths.h, without a GPU: its error bound eps(E) against an
emulation of the screening arithmetic, the register / LDS budget of every instantiation, and the two entry points' binding."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import abi_header
from oracle import vq as ovq
from vq_screen_cases import FINITE_CASES, ROOT, make_case, table_widths

WIDTHS = table_widths()


def eps_bound(E, xnorm, emax):
    """eps_n(E) of csrc/vq_screen.hip (VQ_EPS_K1 and vq_eps_k2<E>() there; derivation in that file's opening comment), without
    the 1.0001 the kernel puts on both norms: what the kernel uses is never smaller."""
    return 8e-5 * xnorm * emax + 1e-5 * ((2 * E + 8) / 136) * (xnorm + emax) ** 2


def test_the_table_and_the_default_width_constants():
    assert WIDTHS == [16, 32, 64, 128, 256]
    assert eps_bound(64, 1.0, 0.0) == 1e-5 and eps_bound(64, 1.0, 1.0) == 8e-5 + 1e-5 * 4        # the E = 64 constants stay


def _split(t):
    """bf16 head and tail of an fp32 tensor, both as fp32 (round to nearest even, as f32_to_bf16_bits)"""
    h = t.to(torch.bfloat16).float()
    return h, (t - h).to(torch.bfloat16).float()


def _screen_values(x, cb):
    """a~(n, c) in three accumulation orders: [3, N, C] fp32.  Terms per 16-wide k-step as the kernel issues them (eh.xh, el.xh,
    eh.xl: exact fp32 products of bf16 factors), start value -|e|^2 / 2 (fp32, sixteen-element chains then a tree)."""
    N, E = x.shape
    xh, xl = _split(x)
    eh, el = _split(cb)
    s = torch.zeros(cb.shape[0], E // 16)
    for i in range(16):
        s = s + cb.view(-1, E // 16, 16)[:, :, i] ** 2
    while s.shape[1] > 1:
        s = s[:, 0::2] + s[:, 1::2]
    nh = -0.5 * s[:, 0]
    terms = []
    for ks in range(E // 16):
        k = slice(16 * ks, 16 * ks + 16)
        for a, b in ((eh, xh), (el, xh), (eh, xl)):
            terms.append(b[:, None, k] * a[None, :, k])              # [N, C, 16]
    P = torch.cat(terms, dim=-1)                                     # [N, C, 3 E]
    up = nh[None].expand(N, -1).clone()
    down = up.clone()
    for t in range(P.shape[-1]):
        up = up + P[:, :, t]
        down = down + P[:, :, P.shape[-1] - 1 - t]
    pair = torch.cat([P, P.new_zeros(N, cb.shape[0], (1 << (P.shape[-1] - 1).bit_length()) - P.shape[-1])], dim=-1)
    while pair.shape[-1] > 1:
        pair = pair[..., 0::2] + pair[..., 1::2]
    return torch.stack([up, down, nh[None] + pair[..., 0]])


@pytest.mark.parametrize('E', WIDTHS)
def test_error_bound_holds_on_the_emulated_screening(E):
    """max |a~ - A| <= eps(E), A(c) = (|x|^2 - d_pinned(c)) / 2 with the pinned fp32 distances of the oracle and the rest in fp64,
    on every finite adversarial case at N = 512, C = 100."""
    N, C = 512, 100
    worst = 0.0
    for case in FINITE_CASES:
        x, cb = make_case(case, N, C, E)
        d_pinned = ovq.distances(x, cb[None])[:, 0].double()
        A = (x.double().pow(2).sum(-1)[:, None] - d_pinned) / 2
        eps = eps_bound(E, x.double().norm(dim=-1), float(cb.double().norm(dim=-1).max()))[None, :, None]
        ratio = float(((_screen_values(x, cb).double() - A[None]).abs() / eps).max())
        print(f'[vq screen bound] E={E} {case}: worst |a~ - A| / eps = {ratio:.3f}')
        worst = max(worst, ratio)
    print(f'[vq screen bound] E={E}: worst ratio {worst:.3f}')
    assert worst <= 1.0


def _resources():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'kres.py'), os.path.join(ROOT, 'world_modelz_amd', 'csrc', 'vq_screen.hip')],
                       capture_output=True, text=True)
    rows = {}
    for line in r.stdout.splitlines():
        t = line.replace('void ', '').split()
        rows[t[0]] = {t[i]: int(t[i + 1]) for i in range(1, len(t) - 1, 2) if t[i] in ('vgpr', 'agpr', 'scratch', 'lds')}
    return r, rows


def test_resource_budget_of_every_instantiation():
    """No instantiation uses scratch or more than 160 KB of LDS, and the default width keeps the registers and LDS it had as the
    only width.  (The re-check kernels' LDS is dynamic: vq_geo<E>::RC_LDS, held to 160 KB by a static_assert next to it.)"""
    r, rows = _resources()
    assert r.returncode == 0, r.stdout + r.stderr             # (kres exits 1 when any kernel spills)
    assert sorted(rows) == sorted(f'{k}<{E}>' for k in ('vq_prep_kernel', 'vq_screen_kernel', 'vq_recheck_kernel') for E in WIDTHS)
    for name, row in rows.items():
        print(name, row)
        assert row['scratch'] == 0, name
        assert row['lds'] <= 160 * 1024, name
    scr, rec = rows['vq_screen_kernel<64>'], rows['vq_recheck_kernel<64>']
    assert scr['vgpr'] <= 140 and scr['agpr'] <= 32 and scr['lds'] <= 37376
    assert rec['vgpr'] + rec['agpr'] <= 185
    with open(os.path.join(ROOT, 'world_modelz_amd', 'csrc', 'vq_screen.hip')) as f:
        assert 'static_assert(RC_LDS <= 160 * 1024' in f.read()


def test_entry_points_are_declared_and_bound():
    from world_modelz_amd import _lib
    vp, i, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    assert _lib.DECLARATIONS['wmz_vq_argmin_screened_workspace_bytes'] == (l, [i, i, i])
    assert _lib.DECLARATIONS['wmz_vq_argmin_screened'] == (i, [vp, l, vp, vp, vp, i, i, i, vp, l, vp])
    for name in ('wmz_vq_argmin_screened_workspace_bytes', 'wmz_vq_argmin_screened'):
        assert abi_header.arguments(name, abi_header.HEADER).count(',') + 1 == len(_lib.SIGNATURES[name])
    assert abi_header.constants('WMZ_VERSION')['WMZ_VERSION'] == _lib.EXPECTED_VERSION
