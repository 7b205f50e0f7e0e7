"""The half guard of the precise mode (config.half_guard; DESIGN 4.7 "Range"): host side.

The half per-token kernels OR the kind of value whose rounding to IEEE half left +-65504 into one device word (include/wmz.h
wmz_half_guard_bind).  A guarded call clears that word on its stream, runs, and reads it back once -- the call's only
synchronisation -- then raises or runs again on the fp32 route, as the policy says.  Guarded calls nest (the model's forward inside a
GraphedForward capture warm-up, the graph replays inside sample_frames): only the outermost one clears and reads.
"""
import contextlib
import threading
import warnings

import torch

from . import _lib as L
from . import config

KINDS = ((L.CONSTANTS['WMZ_HG_STREAM'], 'the residual stream'), (L.CONSTANTS['WMZ_HG_QKV'], 'q / k | v'),
         (L.CONSTANTS['WMZ_HG_CONV'], 'a conv activation'))

_words = {}          # device index -> the bound word (int32[1])
_tls = threading.local()          # .depth > 0: this thread is inside a guarded call (or suspended)


def _bind(dev):
    w = _words.get(dev.index)
    if w is None:
        with torch.cuda.device(dev):
            torch.cuda.synchronize()                            # (the bind is a synchronous symbol copy: nothing in flight reads it)
            w = torch.zeros(1, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            L.call('wmz_half_guard_bind', L.ptr(w))
        _words[dev.index] = w
    return w


def unbind():
    """No word on any device: the kernels skip their tests.  Not called by a change of policy -- a word once bound stays bound for
    the process (the kernels' tests then run under 'off' too and nobody reads the word), so that entering and leaving
    config.half_guard(...) costs no synchronisation; for bit-identity checks against a library without the guard, and tools."""
    for idx in list(_words):
        with torch.cuda.device(idx):
            torch.cuda.synchronize()
            L.call('wmz_half_guard_bind', None)
        del _words[idx]


@contextlib.contextmanager
def suspended():
    """Calls inside are not guarded on their own (a capture warm-up; the body of an outer guarded call)."""
    _tls.depth = getattr(_tls, 'depth', 0) + 1
    try:
        yield
    finally:
        _tls.depth -= 1


def wanted():
    """True when a call made now has to be guarded: the precise mode, a policy other than 'off', not inside another guarded call
    or a stream capture (a capture cannot synchronise: the replay is what gets guarded, graph.GraphedForward)."""
    return (getattr(_tls, 'depth', 0) == 0 and config.get_half_guard() != 'off' and config.is_precise()
            and not torch.cuda.is_current_stream_capturing())


def describe(kinds):
    return ' and '.join(name for bit, name in KINDS if kinds & bit) or f'kind {kinds:#x}'


def guarded(site, owner, dev, half_call, fp32_call=None):
    """half_call() under the guard.  fp32_call: what 'fallback' runs instead, inside config.compute_dtype(float32) (default:
    half_call again -- the same call, which then takes the fp32 route)."""
    if not wanted():
        return half_call()
    dev = torch.device(dev)
    w = _bind(dev)
    L.call('wmz_half_guard_clear', L.ptr(w), L.stream())
    with suspended():
        y = half_call()
    kinds = int(w.item())                                        # the one read-back of the call
    if kinds == 0:
        return y
    if config.get_half_guard() == 'raise':
        raise L.WmzError(f'{site}: {describe(kinds)} left the range of IEEE half (+-65504) in the precise mode; '
                         "config.half_guard('fallback') runs such a call on the fp32 route instead")
    warned = owner.__dict__.setdefault('_wmz_half_guard_warned', set())       # (kept on the model: it dies with it)
    if site not in warned:
        warned.add(site)
        warnings.warn(f'{site}: {describe(kinds)} left the range of IEEE half (+-65504) in the precise mode: running this call on '
                      'the fp32 route (warned once per call site and model)', RuntimeWarning, stacklevel=3)
    with suspended(), config.compute_dtype(torch.float32):
        return (fp32_call or half_call)()


def with_buffers_restored(owner, call):
    """call() after the buffers of `owner` (BatchNorm running statistics a half pass moved) are back at what they are NOW: the
    fallback of a pass with training-mode BatchNorm starts from the state the half pass started from."""
    bufs = list(owner.buffers())
    saved = [b.clone() for b in bufs]

    def again():
        with torch.no_grad():
            for b, s in zip(bufs, saved):
                b.copy_(s)
        return call()
    return again
