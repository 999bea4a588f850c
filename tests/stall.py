"""Bounded stalls for the ordering tests (tests/test_gpu_streams_*.py).

At test shapes every producer finishes long before its consumer starts, so a
missing event, a launch on the wrong stream or a pinned row reused too early
gives the right bits anyway.  A `Stall` puts a bounded busy kernel in front of
one side of a hand-off; whatever is ordered only by luck then runs in the wrong
order every time.

    Stall(stream, ms)       a busy kernel of about `ms` milliseconds on
                            `stream` and an event behind it; pending() says
                            whether it still runs.  Never longer than MAX_MS =
                            500 ms: a quarter of the 2 s bounded flag waits of
                            the persistent launches, so a stall cannot be taken
                            for an expired wait.  The kernel counts clock
                            cycles (torch.cuda._sleep; without it a chain of
                            matmuls of the calibrated length): nothing spins on
                            a flag the host would have to release.
    first_rung(attempt)     attempt(ms) for ms in RUNGS until it returns True:
                            its PRECONDITION held, i.e. the stall was still
                            pending where the stalled side was supposed to be
                            overtaken.  attempt asserts its results at every
                            rung (they must be right whether or not the stall
                            lasted); if the precondition holds at no rung the
                            test FAILS: a stall that ended early proves
                            nothing, and a call that waits for the device
                            never lets it hold.
    concurrent_stream(*others)
                            a torch stream that really runs beside every
                            stream of `others`: with few hardware queues two
                            torch streams can share one, and a stall on one
                            then holds the other back as well.  Streams are
                            drawn from torch's pool until a probe shows B's
                            event complete while A's stall is pending; after
                            POOL = 32 draws the test fails.
    spy(lib)                the names of the stream-taking entries called
                            inside the block: a test that claims an entry in
                            a THROUGH_HOST table asserts that it ran.

The calibration (clock cycles per millisecond, measured once per session with
events) goes to stall_calibration.json, beside the parity tests' error logs
(test_gpu_fullsize._log, as tests/test_gpu_saturation.py).  Stall length is not an
acceptance number; nothing here asserts a time.
"""
import contextlib
import os
import re

import pytest
import torch

import guard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_MS = 500
RUNGS = (10, 40, 160, 500)
POOL = 32                                # torch's streams per priority

_cal = {}


def _calibrate():
    """cycles of torch.cuda._sleep (or matmuls of the fallback chain) per
    millisecond, from one timed call behind a warm-up call."""
    if _cal:
        return _cal
    a, b = torch.cuda.Event(enable_timing=True), \
        torch.cuda.Event(enable_timing=True)
    if hasattr(torch.cuda, '_sleep'):
        probe = 2000000
        torch.cuda._sleep(probe)
        torch.cuda.synchronize()
        a.record()
        torch.cuda._sleep(probe)
        b.record()
        torch.cuda.synchronize()
        _cal.update(kind='sleep', units_per_ms=probe / a.elapsed_time(b))
    else:
        m = torch.ones((2048, 2048), device='cuda')
        probe = 8
        for _ in range(2):
            a.record()
            for _ in range(probe):
                m = (m @ m) * 0.0 + 1.0
            b.record()
            torch.cuda.synchronize()
        _cal.update(kind='matmul', units_per_ms=probe / a.elapsed_time(b),
                    operand=m)
    # what a 10 ms stall then measures (recorded, not asserted)
    a.record()
    _enqueue(10)
    b.record()
    torch.cuda.synchronize()
    from test_gpu_fullsize import _log as log_json
    log_json('calibration',
             {'kind': _cal['kind'], 'units_per_ms': _cal['units_per_ms'],
              'measured_ms_of_a_10_ms_stall': a.elapsed_time(b),
              'max_ms': MAX_MS, 'rungs': RUNGS,
              'device': torch.cuda.get_device_name()},
             'stall_calibration.json')
    return _cal


def _enqueue(ms):
    """the busy kernel(s) on the current stream"""
    n = max(1, int(ms * _cal['units_per_ms']))
    if _cal['kind'] == 'sleep':
        torch.cuda._sleep(n)
    else:
        m = _cal['operand']
        for _ in range(n):
            m = (m @ m) * 0.0 + 1.0


class Stall(object):
    def __init__(self, stream, ms):
        assert 0 < ms <= MAX_MS, ms
        _calibrate()
        self.stream, self.ms = stream, ms
        self.event = torch.cuda.Event()
        with torch.cuda.stream(stream):
            _enqueue(ms)
            self.event.record(stream)

    def pending(self):
        return not self.event.query()


def first_rung(attempt):
    """See the module docstring.  Returns the rung that held."""
    for ms in RUNGS:
        if attempt(ms):
            return ms
    pytest.fail('the precondition held at no rung of %s ms: the stall was '
                'over (or the call waited for the device) where the stalled '
                'side was to be overtaken' % (RUNGS,))


# ------------------------------------------------------------------ streams
_probe_buf = {}
_found = {}


def _runs_beside(a, b):
    """b's trivial work completes while a stall on a is pending"""
    torch.cuda.synchronize()
    buf = _probe_buf.setdefault('t', torch.zeros(64, device='cuda'))
    for ms in RUNGS[:2]:
        st = Stall(a, ms)
        ev = torch.cuda.Event()
        with torch.cuda.stream(b):
            buf.add_(1.0)
            ev.record(b)
        ok = False
        while st.pending():
            if ev.query():
                ok = st.pending()
                break
        torch.cuda.synchronize()
        if ok:
            return True
    return False


def concurrent_stream(*others):
    """See the module docstring.  The answer for a set of streams is kept for
    the session (a test module holds three or four streams, not a new one per
    test)."""
    key = tuple(s.cuda_stream for s in others)
    if key in _found:
        return _found[key]
    tried = set()
    for _ in range(POOL):
        s = torch.cuda.Stream()
        if s.cuda_stream in tried or s.cuda_stream in key:
            continue
        tried.add(s.cuda_stream)
        if all(_runs_beside(o, s) and _runs_beside(s, o) for o in others):
            _found[key] = s
            return s
    pytest.fail('no stream of torch\'s pool (%d draws) runs beside %r'
                % (POOL, others))


# --------------------------------------------------------------------- bits
def bits(t):
    """t's bits as an integer tensor (a copy)"""
    return t.detach().clone().contiguous().view(guard._INT_OF[t.dtype])


def body_fill(t):
    """t (float32) filled with the arena's BODY pattern: a NaN no kernel
    stores, so a word that was never written is seen"""
    t.view(torch.int32).fill_(guard._signed(guard.BODY32, 32))


# ---------------------------------------------------------------------- spy
def stream_entries():
    """The wn_* entries of include/wavenet_hip.h that take `void* stream`."""
    src = open(os.path.join(ROOT, 'include', 'wavenet_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', ' ', src, flags=re.S)
    out = []
    for m in re.finditer(r'\b(?:int|long)\s+(wn_\w+)\s*\(([^)]*)\)\s*;', src):
        params = [' '.join(p.split()) for p in m.group(2).split(',')]
        if any(re.search(r'\bvoid\s*\*\s*stream$', p) for p in params):
            out.append(m.group(1))
    return out


@contextlib.contextmanager
def spy(lib):
    """The set of stream-taking entries called inside the block, each with
    the stream handles it was given: {name: set of handles}."""
    seen = {}
    names = stream_entries()

    def wrap(name, fn):
        def call(*args):
            seen.setdefault(name, set()).add(args[-1])
            return fn(*args)
        return call
    real = {n: getattr(lib, n) for n in names}
    for n, fn in real.items():
        setattr(lib, n, wrap(n, fn))
    try:
        yield seen
    finally:
        for n, fn in real.items():
            setattr(lib, n, fn)
