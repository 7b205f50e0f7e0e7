"""The sampler's nucleus filter on the host (sample.top_p_logits: what the torch path of sample_frames applies and the law the fused
kernel is held to in test_sampler_filters_gpu.py) against a brute-force fp64 nucleus, and the library's class limit as the Python
side sees it."""
import os
import re

import pytest
import torch

from conftest import ROOT


def brute_force_nucleus(row, p):
    """Kept mask of one row by the definition, in fp64 and without a sort: for every distinct weight t the mass of {w >= t}; the
    LARGEST t whose mass reaches p * total is the threshold, {w >= t} is kept (ties with the weakest member included)."""
    w = (row.double() - row.double().max()).exp()
    total = float(w.sum())
    best = None
    for t in w.unique().tolist():
        if float(w[w >= t].sum()) >= p * total and (best is None or t > best):
            best = t
    return w >= best


@pytest.mark.parametrize('p', [1e-6, 0.3, 0.5, 0.9, 0.999])
def test_top_p_logits_is_the_smallest_most_probable_set(p):
    from world_modelz_amd.sample import top_p_logits
    torch.manual_seed(3)
    logits = torch.randn(24, 37) * 2.5
    logits[5, 7:] = -float('inf')                         # a row top-k has filtered already: the dropped classes weigh nothing
    out = top_p_logits(logits, p)
    for r in range(logits.shape[0]):
        kept = brute_force_nucleus(logits[r], p)
        assert torch.equal(out[r] > -float('inf'), kept), r
        assert torch.equal(out[r][kept], logits[r][kept]), r
        assert bool(kept[logits[r].argmax()])
    if p == 1e-6:
        assert bool(((out > -float('inf')).sum(-1) == 1).all())


def test_top_p_logits_keeps_ties_at_the_boundary_and_p_one_is_the_identity():
    from world_modelz_amd.sample import top_p_logits
    ln = torch.tensor([0.5, 0.2, 0.1, 0.1, 0.1]).log()
    # weights (5, 2, 1, 1, 1) / 10: {5, 2} holds 0.7; 0.75 needs one of the three tied classes, so all three stay
    row = ln[[2, 0, 3, 1, 4]].unsqueeze(0)
    assert (top_p_logits(row, 0.75) > -float('inf')).tolist() == [[True] * 5]
    assert (top_p_logits(row, 0.65) > -float('inf')).tolist() == [[False, True, False, True, False]]
    assert (top_p_logits(row, 0.45) > -float('inf')).tolist() == [[False, True, False, False, False]]
    two = torch.zeros(1, 6)                              # six equal classes: any p keeps all of them
    assert torch.equal(top_p_logits(two, 0.01), two)
    x = torch.randn(3, 11)
    assert top_p_logits(x, 1.0) is x and torch.equal(top_p_logits(x, 1.0), x)


def test_the_class_limit_is_the_librarys():
    """The widest codebook the sampler step takes is stated once, in sampler.hip, and read from the library
    (wmz_sample_tokens_max_classes): sample.py asks ops, and carries no copy of the number."""
    from world_modelz_amd import _lib, ops
    assert _lib.DECLARATIONS['wmz_sample_tokens_max_classes'] == (_lib.c_int, [])
    assert 'wmz_sample_tokens_filtered_dev' in _lib.DECLARATIONS
    assert _lib.SIGNATURES['wmz_sample_tokens_filtered_dev'][5:7] == [_lib.c_float, _lib.c_float]           # top_p, inv_temperature
    assert ops.sample_max_classes() == _lib.lib().wmz_sample_tokens_max_classes() == 16384
    with open(os.path.join(ROOT, 'world_modelz_amd', 'sample.py')) as f:
        assert not re.search(r'16[ _]?384', f.read())
