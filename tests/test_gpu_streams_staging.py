"""Staging streams and rings of pinned host rows under a stall
(tests/stall.py): training.StageIn, InputNoise._stage, DeviceCorpus._perms
and StepLog.fetch_later.

A ring's guard is the `done.synchronize()` in front of a row's re-use.  The
rows' events are wrapped here (_Guard), so that the PRECONDITION is exact: the
stall was still pending when the host reached the guard of a row whose last
copy was still queued.  Without the guard the host rewrites (or reads) the row
while the copy waits behind the stall, and the values differ every time."""
import json

import numpy as np
import pytest
import torch

import corpus_ref as R
import noise_ref
import stall
from util import O

pytestmark = pytest.mark.gpu


class _Guard(object):
    """A ring row's event; logs whether the stall was pending whenever the
    host waits for a copy that was recorded through this wrapper."""

    def __init__(self, event, log, current):
        self.event, self.log, self.current = event, log, current
        self.armed, self.records = False, 0

    def record(self, *a):
        self.event.record(*a)
        self.armed, self.records = True, self.records + 1

    def synchronize(self):
        if self.armed and self.current:
            self.log.append(self.current[-1].pending())
        self.event.synchronize()
        self.armed = False

    def query(self):
        return self.event.query()


def _wrap_rows(rows, log, current):
    """[(host, event)] -> the same rows behind _Guard events (in place where
    the owner keeps a list)"""
    out = [(h, e if isinstance(e, _Guard) else _Guard(e, log, current))
           for h, e in rows]
    rows[:] = out
    return [e for _, e in out]


# ------------------------------------------------------------------ StageIn
SIZES = [(2, 333), (2, 334), (3, 222), (2, 333), (1, 667)]   # one block size


def _batches(seed=0):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1, 1, s).astype(np.float32) for s in SIZES]


def _encode(dev):
    from wavenet.ops import mu_law_encode
    return mu_law_encode(dev, 256)


def _stage_in(*beside):
    """A StageIn whose stream really runs beside the streams `beside` (two
    torch streams can share a hardware queue; the copy, which waits for its
    own stream on the host, would then wait for the consumer's stall too),
    after one call."""
    from wavenet.training import StageIn
    stage = StageIn(torch.device('cuda', torch.cuda.current_device()))
    stage.stream = stall.concurrent_stream(*beside)
    first = np.zeros((2, 8), np.float32)
    _encode(stage(torch.from_numpy(first)))
    assert stage.stream.cuda_stream not in [b.cuda_stream for b in beside]
    torch.cuda.synchronize()
    return stage


def test_stage_in_with_its_stream_stalled(hip_lib):
    """The copy sits behind a stall on StageIn's stream; the consumer on the
    current stream must wait for it.  (The pageable copy itself waits for its
    stream on the host, by design: the precondition is taken before the
    call, and what it was after the call is printed.)"""
    stage = _stage_in(torch.cuda.default_stream())
    host = _batches(1)
    want = [O.mu_law_encode(h, 256) for h in host]

    def attempt(ms):
        st = stall.Stall(stage.stream, ms)
        held = st.pending()
        codes = _encode(stage(torch.from_numpy(host[0])))
        print('stall pending behind the call: %s' % st.pending())
        st2 = stall.Stall(stage.stream, ms)
        held = held and st2.pending()
        more = [_encode(stage(torch.from_numpy(h))) for h in host[1:]]
        torch.cuda.synchronize()
        for got, w in zip([codes] + more, want):
            assert np.array_equal(got.cpu().numpy(), w)
        return held
    stall.first_rung(attempt)


def _five_under_one_stall(stage, s):
    host = _batches(2)
    want = [O.mu_law_encode(h, 256) for h in host]

    def attempt(ms):
        with torch.cuda.stream(s):
            st = stall.Stall(s, ms)
            codes = []
            for h in host:
                # (the staged tensor is dropped at once: its block goes back
                # to the stage stream's pool while the consumer is still
                # queued; record_stream keeps it from being handed out)
                codes.append(_encode(stage(torch.from_numpy(h))))
            held = st.pending()
        torch.cuda.synchronize()
        for got, w in zip(codes, want):
            assert np.array_equal(got.cpu().numpy(), w)
        return held
    stall.first_rung(attempt)


def test_stage_in_five_batches_with_the_consumer_stalled(hip_lib):
    """Five batches back to back while the consuming stream is stalled: the
    allocator must not hand a staged block to the next batch before the
    consumer has read it."""
    default = torch.cuda.default_stream()
    _five_under_one_stall(_stage_in(default), default)


def test_stage_in_under_a_non_default_current_stream(hip_lib):
    default = torch.cuda.default_stream()
    s = stall.concurrent_stream(default)
    with torch.cuda.stream(s):
        stage = _stage_in(default, s)
    _five_under_one_stall(stage, s)


# -------------------------------------------------------- InputNoise._stage
def test_input_noise_ring_wraps_under_a_stall(hip_lib):
    """_RING + 2 codes() calls with different host keys and lengths while the
    stream is stalled: the last two re-use pinned rows whose uploads are still
    queued."""
    from wavenet import input_noise
    B, T, Q, prob, width, seed = 3, 37, 256, 0.5, 3, 99
    calls = input_noise._RING + 2
    rng = np.random.default_rng(4)
    q = rng.integers(0, Q, (B, T)).astype(np.int32)
    keys = [rng.integers(0, 1 << 40, B).astype(np.int64) for _ in range(calls)]
    lens = [np.append(rng.integers(1, T + 1, B - 1), T).astype(np.int32)
            for _ in range(calls)]
    want = [noise_ref.codes_in(q, k, n, Q, prob, width, seed)
            for k, n in zip(keys, lens)]
    qd = torch.from_numpy(q).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.current_stream()

    def attempt(ms):
        noise = input_noise.InputNoise(prob, width, seed)
        log, current = [], []
        current.append(stall.Stall(s, ms))
        got = []
        for i in range(calls):
            if i == input_noise._RING:
                (rows,) = noise._pins.values()
                assert len(rows) == input_noise._RING
                guards = _wrap_rows(rows, log, current)
                for g in guards:
                    g.armed = True           # (recorded under the stall)
            got.append(noise.codes(qd, keys[i], lens[i], Q=Q).clone())
        torch.cuda.synchronize()
        for i, g in enumerate(got):
            assert np.array_equal(g.cpu().numpy(), want[i]), i
        return bool(log) and log[0]
    stall.first_rung(attempt)


# ------------------------------------------------------ DeviceCorpus._perms
def test_corpus_permutation_rows_under_a_stall(hip_lib):
    """Eleven items, batches of eight: consecutive steps change epoch, and a
    new permutation goes up through one of two pinned rows (the second row
    for the epoch a batch runs into, the first when a batch starts in an
    epoch that is not resident: the step order jumps, as a restored run's
    does).  A stall before every step; every batch equals the restatement."""
    from wavenet.corpus import DeviceCorpus
    from test_gpu_corpus import LENGTHS, IDS, SEED, _utterances, _same_bits
    utts, B, order = _utterances(), 8, [0, 1, 2, 6, 7, 3, 4, 8, 9]
    P = len(R.make_items(LENGTHS, 64, 'pieces'))
    assert B < P < 2 * B
    want = []
    for step in order:
        slots, T = R.plan(LENGTHS, 64, 'pieces', SEED, step, B, IDS)
        want.append((R.gather(utts, slots, T), [s[2] for s in slots]))
    s = torch.cuda.current_stream()

    def attempt(ms):
        corpus = DeviceCorpus.from_arrays(utts, IDS, sample_size=64,
                                          crop='pieces', seed=SEED)
        b = corpus.batch(0, B)                 # the rows exist now
        got = [(b.audio.clone(), b.lengths.tolist())]
        torch.cuda.synchronize()
        log, current = [], []
        guards = _wrap_rows(corpus._perm_pin, log, current)
        for step in order[1:]:
            current.append(stall.Stall(s, ms))
            b = corpus.batch(step, B)
            # (a ring of two output buffers: copied before the batch after
            # next takes the memory, on the same stream)
            got.append((b.audio.clone(), b.lengths.tolist()))
        torch.cuda.synchronize()
        assert all(g.records >= 2 for g in guards), \
            [g.records for g in guards]
        for step, ((audio, n), (w, wn)) in enumerate(zip(got, want)):
            assert n == wn and _same_bits(audio, w), step
        return bool(log) and all(log)
    stall.first_rung(attempt)


# ----------------------------------------------------- StepLog.fetch_later
def test_step_log_fetches_under_a_stall(hip_lib, tmp_path):
    """StepLog.step's pattern -- norm and loss issued, then the previous
    step's pair read -- for six steps with a stall in front of each: every
    value logged is the value sent."""
    from wavenet.training import StepLog
    n = 2 + 6                                   # two steps create the slots
    losses = [1.5 + 0.25 * k for k in range(n)]
    norms = [100.0 + k for k in range(n)]
    dl = [torch.tensor(v, device='cuda') for v in losses]
    dn = [torch.tensor(v, device='cuda') for v in norms]
    torch.cuda.synchronize()
    s = torch.cuda.current_stream()
    rung = [0]

    def attempt(ms):
        rung[0] += 1
        logdir = tmp_path / ('log%d' % rung[0])
        log = StepLog(None, str(logdir), 0)
        for k in range(2):
            log.step(k, dl[k], dn[k], 0.0)
        torch.cuda.synchronize()
        seen, current = [], []
        rows = sorted(log.slots.items())
        assert len(rows) == 4
        wrapped = [(h, _Guard(e, seen, current)) for _, (h, e) in rows]
        for (key, _), w in zip(rows, wrapped):
            log.slots[key] = w
        # (step 1 is still held, with the events it was recorded on)
        for k in range(2, n):
            current.append(stall.Stall(s, ms))
            log.step(k, dl[k], dn[k], 0.0)
        log.flush()
        log.close()
        lines = [json.loads(l) for l in
                 open(str(logdir / 'events.jsonl')).read().splitlines()]
        assert [l['step'] for l in lines] == list(range(n))
        assert [l['loss'] for l in lines] == losses
        assert [l['grad_norm'] for l in lines] == norms
        # steps 2 .. n - 2 were read while the step after them was stalled
        assert len(seen) >= n - 3, seen
        return all(seen)
    stall.first_rung(attempt)
