"""The sparse sampler's filters and prompts, the parts that need no GPU: the two entry points in the binding read from
include/wmz.h, and sample_clips' refusals, which come before any device work."""
import pytest
import torch

import abi_header


def test_the_two_entry_points_are_declared_with_the_header_s_argument_counts():
    from world_modelz_amd import _lib
    for name, count in (('wmz_categorical_scatter_filtered', 20), ('wmz_sparse_draw_context_known', 19)):
        restype, argtypes = _lib.DECLARATIONS[name]
        assert restype is _lib.c_int and len(argtypes) == count == abi_header.arguments(name).count(',') + 1, name
    # the old entry points' arguments, in place: the known form appends two, the filtered form inserts its filters behind C
    assert _lib.SIGNATURES['wmz_sparse_draw_context_known'][:17] == _lib.SIGNATURES['wmz_sparse_draw_context']
    old, new = _lib.SIGNATURES['wmz_categorical_scatter'], _lib.SIGNATURES['wmz_categorical_scatter_filtered']
    assert new[:4] == old[:4] and new[4:7] == [_lib.c_int, _lib.c_float, _lib.c_float] and new[7:12] == old[4:9] and new[16:] == old[9:]


class Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.shape = (8, 4, 4)
        self.embedding = torch.nn.Embedding(25, 8)

    def forward(self, tokens, indices):
        raise AssertionError('the model was reached')


@pytest.mark.parametrize('bad', [dict(temperature=0), dict(temperature=-1.0), dict(temperature=float('inf')), dict(sample_topp=0),
                                 dict(sample_topp=1.5), dict(prompt=torch.zeros(2, 8, 4, 5, dtype=torch.int64)),
                                 dict(prompt=torch.zeros(3, 8, 4, 4, dtype=torch.int64)),
                                 dict(prompt=torch.zeros(2, 8, 4, 4, dtype=torch.int32)),
                                 dict(prompt=torch.full((2, 8, 4, 4), 25, dtype=torch.int64)),
                                 dict(prompt=torch.full((2, 8, 4, 4), -1, dtype=torch.int64))], ids=lambda b: next(iter(b)))
def test_sample_clips_refuses_bad_arguments_before_any_device_work(bad, monkeypatch):
    """temperature <= 0 or infinite, sample_topp outside (0, 1], a prompt of another shape or dtype, a prompt token outside
    [0, num_embeddings]: ValueError, with the library not loaded and the model not called (a CPU stand-in, 24 codes)."""
    from world_modelz_amd import _lib
    from world_modelz_amd.sparse_diffusion import sample_clips

    def no_library():
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_lib, 'lib', no_library)
    with pytest.raises(ValueError):
        sample_clips(Stub(), 2, 24, 'neighbors', num_context=32, num_eval_iterations=3, **bad)


def test_evaluate_model_keeps_the_reference_s_positional_signature():
    import inspect
    from world_modelz_amd.sparse_diffusion import evaluate_model, sample_clips
    p = inspect.signature(evaluate_model).parameters
    assert list(p)[:8] == ['device', 'batch_size', 'model', 'decoder_model', 'shape', 'sampling_type', 'num_context', 'num_eval_iterations']
    for fn in (evaluate_model, sample_clips):
        p = inspect.signature(fn).parameters
        for name, default in (('temperature', 1.0), ('sample_topk', -1), ('sample_topp', 1.0), ('prompt', None)):
            assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default == default, (fn.__name__, name)
