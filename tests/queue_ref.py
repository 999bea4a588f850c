"""Host references for the restart queue of wavenet/synthesis.py: plan_queue
restated with a heap, and a fake model whose batched generator is a pure
host function of (seed, the stream's own step, previous code, LC row, GC id),
so that synthesize(schedule='queue')'s timeline, first-code cell, row
alignment and per-admission GC ids can be checked without a device."""
import heapq

import numpy as np
import torch


def plan_queue(lengths, batch, quantum=1):
    """(slot, start, segments, steps, occupancy) of the greedy restart queue:
    items by (-n_u, u), each to the slot free first (ties: lowest slot),
    starting at the next multiple of quantum."""
    n = [int(v) for v in lengths]
    heap = [(0, s) for s in range(batch)]
    slot, start = [None] * len(n), [None] * len(n)
    for u in sorted(range(len(n)), key=lambda u: (-n[u], u)):
        free, s = heapq.heappop(heap)
        t = (free + quantum - 1) // quantum * quantum
        slot[u], start[u] = s, t
        heapq.heappush(heap, (t + n[u], s))
    steps = max(t for t, _ in heap)
    cuts = sorted(set(start))
    segments = [(a, (cuts[i + 1] if i + 1 < len(cuts) else steps) - a)
                for i, a in enumerate(cuts)]
    return slot, start, segments, steps, sum(n) / float(batch * steps)


def fold(row):
    """An LC row as one int (rows of the tests hold small integers)."""
    r = np.asarray(row, np.float64).reshape(-1)
    assert np.isfinite(r).all(), 'a row that must not be read was read'
    return int(np.rint((r * (3 + np.arange(r.size))).sum()))


def draw(Q, seed, t, prev, row, gc):
    """The fake model's next code."""
    h = (int(seed) * 1000003 + t * 7919 + int(prev) * 104729 + row * 31
         + (0 if gc is None else int(gc) + 1) * 15485863)
    return (h ^ (h >> 7)) % Q


def alone(Q, n, seed, first, gc, rows):
    """The stand-alone process of one item: n codes behind `first`; step 0
    sees a zero row, step t row t - 1 (rows: [>= n - 1, Lc] or None)."""
    out, prev = [], int(first)
    for t in range(n):
        r = 0 if rows is None or t == 0 else fold(rows[t - 1])
        prev = draw(Q, seed, t, prev, r, gc)
        out.append(prev)
    return np.asarray(out, np.int32)


def upsample(frames, n, hop):
    """The fake upsampler: row t = frame t // hop times (1 + t % hop)."""
    f = np.asarray(frames, np.float32)
    t = np.arange(n)
    return f[t // hop] * (1 + t % hop)[:, None].astype(np.float32)


class FakeNet(object):
    """generate_batch / continue_generation_batch(restart=) / the two LC
    helpers of WaveNetModel that synthesize uses, on the host.  `log` holds
    (name, position, steps, restart) of every batched call."""

    def __init__(self, Q=64, Lc=0, hop=None, graph_steps=20):
        self.Q, self.Lc = Q, Lc
        self.lc_up, self.lc_hop = hop is not None, hop or 1
        self.fastgen_graph_steps = graph_steps
        self.device = 'cpu'
        self.log, self.reserve = [], None
        self.pos, self.t = None, None

    def _rows(self, lc, B, n):
        if not self.Lc:
            assert lc is None
            return None
        lc = lc.numpy()
        assert lc.shape == (B, n, self.Lc) and lc.dtype == np.float32
        return lc

    def _steps(self, last, seeds, gc, lc, n):
        B = len(seeds)
        out = np.zeros((B, n), np.int32)
        prev = np.asarray(last, np.int64).copy()
        for j in range(n):
            for b in range(B):
                r = 0 if lc is None else fold(lc[b, j])
                prev[b] = draw(self.Q, seeds[b], self.t[b] + j, prev[b], r,
                               None if gc is None else gc[b])
                out[b, j] = prev[b]
        self.t = [t + n for t in self.t]
        self.pos += n
        return out

    def _reserved(self, reserve_steps, n):
        assert reserve_steps is not None and reserve_steps >= n
        assert self.reserve in (None, reserve_steps)   # one value per run
        self.reserve = reserve_steps

    def generate_batch(self, num_samples, seeds, seed_samples=None,
                       temperature=1.0, global_condition=None,
                       return_proba_every=0, *, local_condition=None,
                       top_k=None, top_p=None, reserve_steps=None):
        B, n = len(seeds), int(num_samples)
        first = np.asarray(seed_samples)
        assert first.shape == (B, 1)
        self.reserve = None
        self._reserved(reserve_steps, n)
        self.pos, self.t = 0, [0] * B
        self.log.append(('generate_batch', 0, n, None))
        out = self._steps(first[:, 0], seeds, global_condition,
                          self._rows(local_condition, B, n), n)
        return torch.from_numpy(np.concatenate([first.astype(np.int32), out],
                                               axis=1))

    def continue_generation_batch(self, num_samples, last_samples, seeds,
                                  temperature=1.0, global_condition=None,
                                  return_proba_every=0, *,
                                  local_condition=None, top_k=None,
                                  top_p=None, restart=None,
                                  reserve_steps=None):
        B, n = len(seeds), int(num_samples)
        assert B == len(self.t)
        self._reserved(reserve_steps, n)
        self.log.append(('continue_generation_batch', self.pos, n,
                         None if restart is None else list(restart)))
        for b in restart or []:
            self.t[b] = 0
        last = last_samples.numpy()
        assert last.shape == (B,)
        return torch.from_numpy(self._steps(
            last, seeds, global_condition,
            self._rows(local_condition, B, n), n))

    def upsample_local_condition(self, frames, num_samples, offset=0):
        assert offset == 0
        return torch.from_numpy(upsample(frames, int(num_samples),
                                         self.lc_hop))

    def batch_local_condition(self, items, position, num_steps):
        assert position == (self.pos or 0)
        out = np.zeros((len(items), num_steps, self.Lc), np.float32)
        for b, it in enumerate(items):
            if it is None:
                continue
            rows, origin = it
            rows = rows.numpy()
            assert rows.flags['C_CONTIGUOUS'] and rows.dtype == np.float32
            for j in range(num_steps):
                t = position + j - origin
                if 1 <= t <= rows.shape[0]:
                    out[b, j] = rows[t - 1]
        return torch.from_numpy(out)
