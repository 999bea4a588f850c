"""include/wavenet_hip.h promises that every entry is "asynchronous on the
caller's `stream` ... no internal synchronisation".  Every row of
tests/test_gpu_guard_entries.py (its first, smallest case) runs here on a
STALLED stream that is not the default stream (tests/stall.py):

  * no internal synchronisation: every call has returned its code and the
    stall is still pending;
  * it ran nowhere else: an observer stream that really runs beside the
    stalled one (stall.concurrent_stream) copies the outputs and is waited
    for -- every output word still holds what it held before the calls (the
    arena's BODY pattern for an `out` operand), and the stall is still
    pending afterwards.  A launch that strayed onto the null stream, or onto
    any stream but the caller's, has run by then;
  * same result: once the stream has drained, the outputs equal those of the
    same calls on the default stream bit for bit, and no band was touched.

Two runs on the default stream give the reference; an entry whose two
default-stream runs differ in bits is not deterministic and is listed in
TOLERANCE with its parity test's bound (none so far).

The persistent stack launches and the fast-generation family have no row;
tests/test_gpu_streams_training.py and tests/test_gpu_streams_generation.py
run them through the host (THROUGH_HOST there, tests/test_streams_host.py)."""
import pytest
import torch

import stall
from test_gpu_guard_entries import ROWS, Ctx, run_calls, _short

pytestmark = pytest.mark.gpu

# entry -> (rtol, atol) of its parity test, for an entry whose default-stream
# runs are not bit-equal
TOLERANCE = {}

CASES = [pytest.param(r, r.cases[0], id='%s[%s]' % (r.entry, _short(r.cases[0])))
         for r in ROWS]


def _default_stream_run(lib, row, case):
    c = Ctx(lib)
    calls = row.build(c, **case)
    code = run_calls(c, calls)
    torch.cuda.synchronize()
    assert code == c.expect, (row.entry, code)
    return c.a.snapshot()


def _same(row, name, got, ref):
    if row.entry in TOLERANCE:
        rtol, atol = TOLERANCE[row.entry]
        f = {torch.int32: torch.float32, torch.int64: torch.float64}[got.dtype]
        assert torch.allclose(got.view(f), ref.view(f), rtol, atol), \
            (row.entry, name)
        return
    bad = got != ref
    assert not bool(bad.any()), \
        '%s: output %r differs from the default-stream run in %d word(s), ' \
        'first at %d' % (row.entry, name, int(bad.sum()),
                         int(torch.nonzero(bad.reshape(-1))[0]))


@pytest.mark.parametrize('row,case', CASES)
def test_entry_on_a_stalled_stream(hip_lib, row, case):
    ref = _default_stream_run(hip_lib, row, case)
    again = _default_stream_run(hip_lib, row, case)
    if row.entry not in TOLERANCE:
        for name in ref:
            assert torch.equal(ref[name], again[name]), \
                '%s: two default-stream runs differ in %r: not ' \
                'deterministic, compare it at tolerance' % (row.entry, name)
    s = stall.concurrent_stream(torch.cuda.default_stream())
    obs = stall.concurrent_stream(torch.cuda.default_stream(), s)

    def attempt(ms):
        with torch.cuda.stream(s):
            c = Ctx(hip_lib)
            assert c.st == s.cuda_stream != \
                torch.cuda.default_stream().cuda_stream
            calls = row.build(c, **case)
            before = c.a.snapshot()
            torch.cuda.synchronize()
            st = stall.Stall(s, ms)
            code = run_calls(c, calls)
            returned = st.pending()
        assert code == c.expect, (row.entry, code)
        with torch.cuda.stream(obs):
            seen = c.a.snapshot()
        obs.synchronize()
        overtaken = st.pending()
        s.synchronize()
        if returned and overtaken:
            for name, b in before.items():
                bad = seen[name] != b
                assert not bool(bad.any()), \
                    '%s: %d word(s) of %r were written while the caller\'s ' \
                    'stream was stalled: a launch ran on another stream' \
                    % (row.entry, int(bad.sum()), name)
        got = c.a.snapshot()
        torch.cuda.synchronize()
        for name in ref:
            _same(row, name, got[name], ref[name])
        c.a.check()
        if c.expect == 0:
            assert any(bool((got[n] != before[n]).any()) for n in got), \
                '%s wrote nothing' % row.entry
        return returned and overtaken
    stall.first_rung(attempt)


# ---- entries without a row that a thin host wrapper launches ---------------
# (EXEMPT in tests/test_gpu_guard_entries.py: their band tests live in their
# own modules.)  The wrapper runs on torch's current stream; where it takes
# `out=` the output is observed like a row's, and stall.spy says which stream
# handle the entry was given.
def _w_melspec(x, out):
    from wavenet import features
    spec = _w_melspec.spec = getattr(_w_melspec, 'spec', None) or \
        features.MelSpec(16000, n_fft=64, hop=16, n_mels=12)
    return [spec(x['audio'])]


def _w_stats(x, out):
    from wavenet import features
    s = features.FeatureStats(12).update(x['frames'])
    return [s._acc]


def _w_normalize(x, out):
    from wavenet import features
    nz = _w_normalize.nz = getattr(_w_normalize, 'nz', None) or \
        features.Normalizer.from_range(-2.0, 2.0, 12)
    return [nz(x['frames'], out=out['frames'])]


def _w_distance(x, out):
    from wavenet import features
    return list(features.frame_distance(x['frames'], x['frames2']))


def _w_pre(x, out):
    from wavenet import emphasis
    return [emphasis.Emphasis(0.97).pre(x['audio'], out=out['audio'])]


def _w_de(x, out):
    from wavenet import emphasis
    return list(emphasis.Emphasis(0.97).de(x['audio'], out=out['audio'],
                                           return_last=True))


# entry -> (wrapper, the `out=` it takes or None); 3 clips of 333 samples,
# 3 x 21 frames of 12 channels: more than one workgroup of each kernel
THROUGH_HOST = {
    'wn_melspec': (_w_melspec, None),
    'wn_feature_stats': (_w_stats, None),
    'wn_feature_normalize': (_w_normalize, 'frames'),
    'wn_feature_distance': (_w_distance, None),
    'wn_preemphasis': (_w_pre, 'audio'),
    'wn_deemphasis': (_w_de, 'audio'),
}


def _w_inputs():
    g = torch.Generator().manual_seed(5)
    return {'audio': (torch.rand((3, 333), generator=g) * 2 - 1).cuda(),
            'frames': torch.randn((3, 21, 12), generator=g).cuda(),
            'frames2': torch.randn((3, 21, 12), generator=g).cuda()}


def _w_out(x, name):
    if name is None:
        return {}
    t = torch.empty_like(x[name])
    stall.body_fill(t)
    return {name: t}


@pytest.mark.parametrize('entry', sorted(THROUGH_HOST))
def test_wrapped_entry_on_a_stalled_stream(hip_lib, entry):
    fn, out_name = THROUGH_HOST[entry]
    x = _w_inputs()
    ref = [stall.bits(t) for t in fn(x, _w_out(x, out_name))]
    again = [stall.bits(t) for t in fn(x, _w_out(x, out_name))]
    torch.cuda.synchronize()
    for a, b in zip(ref, again):
        assert torch.equal(a, b), entry
    s = stall.concurrent_stream(torch.cuda.default_stream())
    obs = stall.concurrent_stream(torch.cuda.default_stream(), s)

    def attempt(ms):
        out = _w_out(x, out_name)
        before = {k: stall.bits(v) for k, v in out.items()}
        torch.cuda.synchronize()
        with torch.cuda.stream(s), stall.spy(hip_lib) as seen:
            st = stall.Stall(s, ms)
            res = fn(x, out)
            returned = st.pending()
        assert seen.get(entry) == {s.cuda_stream}, (entry, seen)
        with torch.cuda.stream(obs):
            early = {k: stall.bits(v) for k, v in out.items()}
        obs.synchronize()
        overtaken = st.pending()
        s.synchronize()
        if returned and overtaken:
            for k in before:
                assert torch.equal(early[k], before[k]), \
                    '%s: %r was written while its stream was stalled' \
                    % (entry, k)
        for a, t in zip(ref, res):
            assert torch.equal(a, stall.bits(t)), entry
        return returned and overtaken
    stall.first_rung(attempt)
