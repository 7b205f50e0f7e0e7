"""Operand-dtype copies of fp32 parameters (and anything else built from them), cached until a parameter changes.

An entry is `(stamp, value, weak references to the parameters)` under the key `(tag, dtype, id() of each parameter)`.  It is
served only while all of this holds (_stamp_of and _current, the one implementation of the rule):
  - the global epoch has not moved (invalidate(): weights rewritten behind torch's version counters);
  - every parameter's `_version` is the one the entry was stored at (in-place writes: optimizer step, load_state_dict);
  - every parameter's `data_ptr()` is (re-allocation: .to(), `p.data = ..`);
  - the weak references still point at these very objects: the key is made of id()s, and a freed parameter's id (and storage
    address, and version) can come back with another model's tensor.
operand() and cached() build a missing or stale entry themselves; stamp() records a value that a bulk refresher (BulkOperands,
ConvOperands, fused.PackSet) has just rebuilt into its own persistent buffer, so that the getters hit."""
import weakref

import torch

_cache = {}
_epoch = 0      # bumped when parameters are rewritten behind torch's version counters (arena optimizer step)


def _key(ts, dtype, tag):
    return (tag, dtype) + tuple(id(t) for t in ts)


def _stamp_of(params):
    return (_epoch,) + tuple((p._version, p.data_ptr()) for p in params)


def _current(hit, params):
    """Is this cache hit the value of these very objects, as they are now?"""
    return hit is not None and hit[0] == _stamp_of(params) and all(r() is p for r, p in zip(hit[2], params))


def _store(key, params, value):
    _sweep()
    _cache[key] = (_stamp_of(params), value, tuple(weakref.ref(p) for p in params))
    return value


def stamp(params, dtype, tag, value):
    """Record `value` -- rebuilt from `params` as they are now by someone else's launch, into a buffer that persists -- as the
    current entry operand(params, dtype, tag, ..) looks up (dtype None: cached(params, tag, ..))."""
    params = tuple(params)
    _store(_key(params, dtype, tag), params, value)


def held():
    """The values the cache holds now (tensors or tuples of tensors): what a captured graph keeps strong references to."""
    return [h[1] for h in _cache.values()]


def operand(params, dtype, tag='w', build=None):
    """Return `build(*params)` (default: the single parameter itself) cast to `dtype`, contiguous, cached until
    any of the parameters is modified in place (optimizer step, load_state_dict) or re-allocated (.to())."""
    if not isinstance(params, (tuple, list)):
        params = (params,)
    if build is None and len(params) == 1 and params[0].dtype == dtype and params[0].is_contiguous():
        return params[0].detach()
    return _get(params, dtype, tag, build, True)


def cached(params, tag, build):
    """Like operand(), for values that are not a single cast tensor: `build(*params)` is kept until any parameter changes."""
    return _get(tuple(params), None, tag, build, False)


def _get(params, dtype, tag, build, cast):
    key = _key(params, dtype, tag)
    hit = _cache.get(key)
    if _current(hit, params):
        return hit[1]
    with torch.no_grad():
        val = build(*params) if build is not None else params[0]
        if cast:
            val = val.detach().to(dtype).contiguous()
    return _store(key, params, val)


_sweep_at = 256


def _sweep():
    """Drop the entries of parameters that no longer exist (a model that was deleted leaves ~10 MB of operand copies per 3 M
    parameters behind).  Runs when the cache has doubled since the last sweep (at least 256 entries): amortised O(1) per insert."""
    global _sweep_at
    if len(_cache) < _sweep_at:
        return
    for k in [k for k, h in _cache.items() if any(r() is None for r in h[2])]:
        del _cache[k]
    _sweep_at = max(256, 2 * len(_cache))


_scoped = {}       # id(parameter) -> [weakref to it, how often invalidate(params) named it]
_unscoped = 0      # invalidate() calls that named nothing
_scoped_sweep_at = 1024


def invalidate(params=None):
    """Parameters changed in place without torch noticing (wmz_adamw_step on the flat arena).  Every operand copy is rebuilt at its
    next use either way (the global epoch moves); `params` says WHOSE weights moved, for holders of captured graphs: a graph
    re-captures only when its own model's tensors were named (graph.GraphedForward: the frozen auto-encoder's encoder graph must
    survive the denoiser's optimizer steps -- main.py:229-287 runs both in every training step)."""
    global _epoch, _unscoped, _scoped_sweep_at
    _epoch += 1
    if params is None:
        _unscoped += 1
        return
    for p in params:
        e = _scoped.get(id(p))
        # (the key is an id(): a freed parameter's id can come back with another model's tensor -- an entry counts only while its
        #  weak reference still points at this very object, like _cache's)
        if e is None or e[0]() is not p:
            _scoped[id(p)] = [weakref.ref(p), 1]
        else:
            e[1] += 1
    if len(_scoped) >= _scoped_sweep_at:
        for k in [k for k, e in _scoped.items() if e[0]() is None]:
            del _scoped[k]
        _scoped_sweep_at = max(1024, 2 * len(_scoped))


def epoch_of(tensors):
    """What a graph holder stamps: moves when invalidate() named one of `tensors` (or named nothing)."""
    n = 0
    for t in tensors:
        e = _scoped.get(id(t))
        if e is not None and e[0]() is t:
            n += e[1]
    return _unscoped, n


def clear():
    _cache.clear()


class BulkOperands:
    """Operand copies that are rebuilt together, by ONE launch of wmz_operands_refresh (training: after every optimizer
    step).  Each entry is registered under the same (params, dtype, tag) key the forward / backward code asks operand()
    for; refresh() fills the persistent destination tensors and records each with stamp(), so those operand() calls hit.
    Anything not registered, or invalidated in another way, still takes the ordinary per-operand path."""

    def __init__(self):
        self.entries = []          # (params, dtype, tag, transpose, zero_first, dst)

    def add(self, params, dtype, tag='w', transpose=False, zero_first=False):
        params = tuple(params)
        rows = sum(p.shape[0] for p in params) + (params[0].shape[0] if zero_first else 0)
        cols = params[0].numel() // params[0].shape[0]
        assert len(params) <= 2 and not (zero_first and len(params) != 1)
        shape = (cols, rows) if transpose else ((rows, cols) if params[0].dim() > 1 else (rows,))
        dst = torch.empty(shape, dtype=dtype, device=params[0].device)
        self.entries.append((params, dtype, tag, transpose, zero_first, dst))
        return dst

    def refresh(self):
        from . import _lib as L
        T, F32 = L.CONSTANTS['WMZ_OPERAND_TRANSPOSE'], L.CONSTANTS['WMZ_OPERAND_F32']
        for i0 in range(0, len(self.entries), 64):
            rows = []           # (source 0 | None = zero rows, source 1 | None, rows 0, rows 1, columns, destination, flags)
            for params, dtype, tag, tr, zf, dst in self.entries[i0:i0 + 64]:
                a = params[0].detach()
                b = params[1].detach() if len(params) > 1 else None
                assert a.dtype == torch.float32 and a.is_contiguous() and (b is None or b.is_contiguous())
                if zf:
                    src = (None, a.data_ptr(), a.shape[0], a.shape[0])
                else:
                    src = (a.data_ptr(), b.data_ptr() if b is not None else None, a.shape[0], b.shape[0] if b is not None else 0)
                rows.append(src + (a.numel() // a.shape[0], dst.data_ptr(),
                                   (T if tr else 0) | (F32 if dtype == torch.float32 else 0)))
            L.call('wmz_operands_refresh', *L.columns(rows, 'ppiiipi'), len(rows), L.stream())
        for params, dtype, tag, tr, zf, dst in self.entries:
            stamp(params, dtype, tag, dst)


class ConvOperands:
    """The conv encoder / decoder's GEMM operands (autoencoder.py: tags 'conv' and 'convT'), rebuilt together by ONE launch of
    wmz_conv_operands_refresh_packed after every optimizer step; refresh() records each with stamp(), so the forward / backward's
    operand() calls hit (built with tensor ops otherwise: permute, pad, flip, cast -- ~6 launches per layer).
    bf16: the same launch also writes the fragment-order weight streams of the direct kernels (csrc/conv_direct.hip,
    csrc/conv_point.hip: ops._direct_pack / ops._point_pack, cached per operand tensor) -- 34 pack launches per step otherwise."""

    def __init__(self, convs, dtype):
        self.dtype = dtype
        self.entries = []          # (weight, tag, mode, pack kind, dst, operand dst the pack belongs to | None)
        for conv in convs:
            w = conv.weight
            co, ci, kh, kw = w.shape
            ci8, co8 = (ci + 7) // 8 * 8, (co + 7) // 8 * 8
            for tag, mode, rows, kin in (('conv', 0, co8, ci8), ('convT', 1, ci8, co8)):
                op = torch.empty((rows, kh * kw * kin), dtype=dtype, device=w.device)
                self.entries.append((w, tag, mode, 0, op, None))
                if dtype != torch.bfloat16 or rows > 128 or rows % 8 != 0:
                    continue
                ncb = 2 if rows <= 64 else 4
                if kh == 3 and kw == 3 and kin in (64, 128):
                    self.entries.append((w, 'convq', mode, 1, torch.empty(9 * kin * ncb * 32, dtype=dtype, device=w.device), op))
                elif kh * kw * kin <= 256:
                    n = (kh * kw * kin + 63) // 64 * 64 * ncb * 32
                    self.entries.append((w, 'convp', mode, 2, torch.empty(n, dtype=dtype, device=w.device), op))

    def refresh(self):
        from . import _lib as L
        for i0 in range(0, len(self.entries), 48):
            rows = []           # (weight, destination, C_out, C_in, kh * kw, mode, pack kind)
            for w, tag, mode, pack, dst, _op in self.entries[i0:i0 + 48]:
                wd = w.detach()
                assert wd.dtype == torch.float32 and wd.is_contiguous()
                rows.append((wd.data_ptr(), dst.data_ptr(), w.shape[0], w.shape[1], w.shape[2] * w.shape[3], mode, pack))
            L.call('wmz_conv_operands_refresh_packed', *L.columns(rows, 'ppiiiii'), len(rows), L.dtype_code(self.dtype), L.stream())
        for w, tag, mode, pack, dst, op in self.entries:
            if pack == 0:
                stamp((w,), self.dtype, tag, dst)
            else:               # keyed by the operand tensor it re-orders (ops._direct_pack / _point_pack -> cached((op,), tag, ..))
                stamp((op,), None, tag, dst)
