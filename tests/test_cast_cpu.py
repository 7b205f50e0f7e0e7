"""The operand cache's validity rule (world_modelz_amd/_cast.py) for entries recorded with stamp(), and _lib.columns: plain CPU
tensors, no library call."""
import ctypes
import gc
import weakref

import pytest
import torch

from world_modelz_amd import _cast, _lib

BF16 = torch.bfloat16


@pytest.fixture(autouse=True)
def _fresh_cache():
    _cast.clear()
    _cast._sweep_at = 256
    yield
    _cast.clear()
    _cast._sweep_at = 256


def _raises(*_):
    raise AssertionError('the stamped value should have been served')


def test_stamped_value_is_served():
    p, a, b = torch.randn(4, 4), torch.randn(3), torch.randn(3)
    v, val = torch.zeros(4, 4, dtype=BF16), (torch.zeros(6), torch.zeros(2))
    _cast.stamp((p,), BF16, 'w', v)
    _cast.stamp((a, b), None, 'x', val)
    assert _cast.operand(p, BF16) is v
    assert _cast.operand((p,), BF16, 'w', _raises) is v
    assert _cast.cached((a, b), 'x', _raises) is val
    assert _cast.cached([a, b], 'x', _raises) is val
    # other keys are not served by them: another tag, another dtype, another order of the parameters
    assert _cast.operand((p,), BF16, 'wT', lambda t: t.t()) is not v
    assert _cast.operand(p, torch.float16) is not v
    assert _cast.cached((b, a), 'x', lambda *ts: 'rebuilt') == 'rebuilt'


STALE = {'in-place write': lambda p: p.add_(1.0),
         'invalidate()': lambda p: _cast.invalidate(),
         'invalidate([p])': lambda p: _cast.invalidate([p]),
         'new storage': lambda p: setattr(p, 'data', p.data.clone())}


@pytest.mark.parametrize('event', list(STALE))
def test_stamped_entry_goes_stale_like_a_built_one(event):
    p, other = torch.randn(4, 4), torch.randn(4, 4)
    v, val = torch.zeros(4, 4, dtype=BF16), (torch.zeros(1),)
    _cast.stamp((p,), BF16, 'w', v)
    _cast.stamp((other, p), None, 'x', val)
    built = _cast.operand((p,), BF16, 'wT', lambda t: t.t())           # an entry the getter built itself: same fate
    STALE[event](p)
    got = _cast.operand(p, BF16)
    assert got is not v and torch.equal(got, p.to(BF16))
    assert _cast.operand(p, BF16) is got                                  # and the rebuilt one is served from then on
    fresh = (torch.ones(1),)
    assert _cast.cached((other, p), 'x', lambda *ts: fresh) is fresh
    rebuilt = _cast.operand((p,), BF16, 'wT', lambda t: t.t())
    assert rebuilt is not built and torch.equal(rebuilt, p.t().to(BF16))


def test_a_key_does_not_serve_another_object():
    """The key is made of id()s.  q shares p's storage and version counter, so p's entry copied under q's key carries the right
    stamp -- what a recycled id looks like -- and only its weak reference tells the two apart."""
    p = torch.randn(4, 4)
    q = p.detach()
    assert q is not p and (q._version, q.data_ptr()) == (p._version, p.data_ptr())
    v = torch.zeros(4, 4, dtype=BF16)
    _cast.stamp((p,), BF16, 'w', v)
    _cast._cache[_cast._key((q,), BF16, 'w')] = _cast._cache[_cast._key((p,), BF16, 'w')]
    got = _cast.operand(q, BF16)
    assert got is not v and torch.equal(got, q.to(BF16))
    assert _cast.operand(p, BF16) is v


def test_held_and_release_with_the_parameter():
    p, other = torch.randn(4, 4), torch.randn(4, 4)
    v = torch.zeros(4, 4, dtype=BF16)
    _cast.stamp((p,), BF16, 'w', v)
    assert any(x is v for x in _cast.held())
    _cast.clear()
    assert not any(x is v for x in _cast.held())

    _cast.stamp((p,), BF16, 'w', v)
    r = weakref.ref(v)
    del v
    gc.collect()
    assert r() is not None                       # the cache is what keeps it
    del p
    gc.collect()
    _cast._sweep_at = 0                          # force a sweep at the next insert
    _cast.stamp((other,), BF16, 'w', torch.zeros(4, 4, dtype=BF16))
    assert r() is None and len(_cast._cache) == 1 and len(_cast.held()) == 1


def test_columns():
    ptrs, ints, longs = _lib.columns([(None, 5, 2 ** 40), (123456789012, -1, 7)], 'pil')
    assert isinstance(ptrs, ctypes.c_void_p * 2) and list(ptrs) == [None, 123456789012]
    assert isinstance(ints, ctypes.c_int * 2) and list(ints) == [5, -1]
    assert isinstance(longs, ctypes.c_long * 2) and list(longs) == [2 ** 40, 7]
    with pytest.raises(AssertionError):
        _lib.columns([(1, 2)], 'pil')
