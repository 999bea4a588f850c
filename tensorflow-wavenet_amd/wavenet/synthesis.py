"""Bulk synthesis: many utterances of different lengths through the batched
generator (WaveNetModel.generate_batch), in rounds of `batch` streams.

The items are sorted by length, longest first (ties by index), and cut into
consecutive groups of `batch`; a round steps its streams in lock step for as
many steps as its longest item has samples, and every shorter stream's codes
behind its own length are dropped (`plan_rounds`).

The contract of `synthesize`: codes[u] equals, bit for bit,

    net.generate_batch(n_u, [seeds[u]], seed_samples=[[first_u]],
                       global_condition=gc_u,
                       local_condition=cat(zeros(1, Lc), rows_u[:n_u - 1])[None],
                       temperature=..., top_k=..., top_p=...)[0, 1:]

with rows_u = net.upsample_local_condition(frames_u, n_u) where frames were
given.  It follows from generate_batch's batch invariance (a stream's codes
do not depend on B or the other streams) and from causality (a stream's code
k does not depend on the rows behind position k); tests/test_gpu_synthesis.py
checks it.  No kernel is launched here but through the model's own methods.

schedule='queue' (`plan_queue`) keeps the contract and drops the rounds: the
items, in the same order, each take the slot that is free first, so a slot
whose item has ended does not idle to the end of a round.  The generator
runs one segment of lock-step steps between consecutive admission times;
at each of them the admitted slots are restarted inside the running batch
(continue_generation_batch's `restart`: zero queues, no previous code, the
draw counted from the stream's own first step), which makes the new item's
stream bit for bit a fresh one.  tests/test_gpu_synthesis_queue.py.
"""
import collections

import numpy as np

from . import _lib, sampling

BATCH_MAX = 256
Plan = collections.namedtuple('Plan', 'rounds steps occupancy')
Synthesis = collections.namedtuple('Synthesis', 'codes rounds steps occupancy')
QueuePlan = collections.namedtuple('QueuePlan',
                                   'slot start segments steps occupancy')
SCHEDULES = ('rounds', 'queue')


def _ints(v, what, lo=None):
    """`v` as int64 numpy [n] (ints, no bools)."""
    if hasattr(v, 'detach'):
        v = v.detach().cpu().numpy()
    a = np.asarray(v)
    if a.ndim == 1 and a.size == 0:
        return np.zeros(0, np.int64)
    if a.ndim != 1 or a.dtype == object or a.dtype == np.bool_ or \
            not np.issubdtype(a.dtype, np.integer):
        raise ValueError('%s must be a list of ints, got %r' % (what, v))
    a = a.astype(np.int64)
    if lo is not None and a.size and int(a.min()) < lo:
        raise ValueError('%s must be >= %d, got %d' % (what, lo, a.min()))
    return a


def _batch(batch):
    if isinstance(batch, (bool, np.bool_)) or \
            not isinstance(batch, (int, np.integer)) or \
            not 1 <= int(batch) <= BATCH_MAX:
        raise ValueError('batch must be an int in [1, %d], got %r'
                         % (BATCH_MAX, batch))
    return int(batch)


def plan_rounds(lengths, batch):
    """The rounds of `lengths` (one int >= 1 per item) at `batch` streams:
    Plan(rounds, steps, occupancy).  rounds: lists of item indices, the items
    in the order (-n_u, u) cut into consecutive groups of `batch`; round r
    runs lengths[rounds[r][0]] lock-step steps; steps: their sum; occupancy =
    sum n_u / (batch * steps), which counts the slots of a full batch also
    where the last round holds fewer items.  Host only."""
    n = _ints(lengths, 'lengths', 1)
    if n.size < 1:
        raise ValueError('lengths must name at least one item')
    B = _batch(batch)
    order = sorted(range(n.size), key=lambda u: (-int(n[u]), u))
    rounds = [order[i:i + B] for i in range(0, len(order), B)]
    steps = sum(int(n[r[0]]) for r in rounds)
    return Plan(rounds, steps, float(n.sum()) / (B * steps))


def _quantum(quantum):
    if isinstance(quantum, (bool, np.bool_)) or \
            not isinstance(quantum, (int, np.integer)) or int(quantum) < 1:
        raise ValueError('quantum must be an int >= 1, got %r' % (quantum,))
    return int(quantum)


def plan_queue(lengths, batch, quantum=1):
    """The restart queue of `lengths` at `batch` slots: QueuePlan(slot,
    start, segments, steps, occupancy).  The items are taken in the order
    (-n_u, u); every slot is free at step 0; an item takes the slot that is
    free first (ties: the lowest slot) and starts at start[u] = its free
    time rounded up to a multiple of `quantum`, which frees the slot at
    start[u] + n_u.  slot, start: one int per item; steps = max(start + n);
    segments: the (a, n) pieces between consecutive distinct start times,
    the last one running to `steps`; occupancy = sum n_u / (batch * steps),
    counted as plan_rounds counts it.  Host only."""
    n = _ints(lengths, 'lengths', 1)
    if n.size < 1:
        raise ValueError('lengths must name at least one item')
    B = _batch(batch)
    q = _quantum(quantum)
    free = [0] * B
    slot, start = [0] * n.size, [0] * n.size
    for u in sorted(range(n.size), key=lambda u: (-int(n[u]), u)):
        s = min(range(B), key=lambda j: (free[j], j))
        slot[u], start[u] = s, -(-free[s] // q) * q
        free[s] = start[u] + int(n[u])
    steps = max(free)
    cuts = sorted(set(start)) + [steps]
    segments = [(a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    return QueuePlan(slot, start, segments, steps,
                     float(n.sum()) / (B * steps))


def _shape_of(t, what):
    if not hasattr(t, 'detach'):
        t = np.asarray(t)
        if t.dtype == object or not np.issubdtype(t.dtype, np.floating):
            raise ValueError('%s must be a float array' % what)
    elif not t.is_floating_point():
        raise ValueError('%s must be floating point' % what)
    return t, tuple(int(v) for v in t.shape)


def _check_lc(net, n, local_condition, frames):
    """The items' rows or frames, checked against the model: (kind, list)."""
    U = n.size
    if local_condition is not None and frames is not None:
        raise ValueError('synthesize: give local_condition (rows at audio '
                         'rate) or frames, not both')
    given = local_condition if local_condition is not None else frames
    if not net.Lc:
        if given is not None:
            raise ValueError('synthesize: this model was built without local '
                             'conditioning (local_condition_channels=None)')
        return None, None
    if net.lc_up:
        if local_condition is not None:
            raise ValueError('synthesize: the model upsamples local '
                             'conditioning (hop %d): pass frames=, not rows'
                             % net.lc_hop)
        if frames is None:
            raise ValueError('synthesize: the model upsamples local '
                             'conditioning (hop %d); frames (one [F, %d] per '
                             'item) are required' % (net.lc_hop, net.Lc))
    else:
        if frames is not None:
            raise ValueError('synthesize: frames are for models built with '
                             'local_condition_upsample_scales; this model '
                             'takes local_condition rows at audio rate')
        if local_condition is None:
            raise ValueError('synthesize: the model was built with local '
                             'conditioning (%d channels); local_condition '
                             '(one [n, %d] per item) is required'
                             % (net.Lc, net.Lc))
    name = 'frames' if net.lc_up else 'local_condition'
    if isinstance(given, np.ndarray) or hasattr(given, 'detach') or \
            len(given) != U:
        raise ValueError('synthesize: %s must be a list of %d arrays, one '
                         'per item' % (name, U))
    out = []
    for u, t in enumerate(given):
        t, shape = _shape_of(t, 'synthesize: %s[%d]' % (name, u))
        need = -(-int(n[u]) // net.lc_hop) if net.lc_up else int(n[u])
        if len(shape) != 2 or shape[1] != net.Lc:
            raise ValueError('synthesize: %s[%d] must have shape [%s, %d], '
                             'got %s' % (name, u, 'F' if net.lc_up else 'n',
                                         net.Lc, shape))
        if shape[0] < need:
            raise ValueError('synthesize: %s[%d] has %d rows, item %d of %d '
                             'samples needs %d' % (name, u, shape[0], u,
                                                   int(n[u]), need))
        out.append(t)
    return name, out


def _device(net, t):
    import torch
    if not isinstance(t, torch.Tensor):
        t = torch.from_numpy(np.ascontiguousarray(t, np.float32))
    return t.to(device=net.device, dtype=torch.float32)


def _round_rows(net, kind, cond, items, n, B, steps):
    """float32 [B, steps, Lc] on the device: stream j's row at position 0 is
    zero (beside the first code), position k + 1 holds row k of its item for
    k < n_u - 1, zeros follow; streams behind len(items) are all zeros."""
    import torch
    Lc = net.Lc
    rows = torch.zeros((B, steps, Lc), dtype=torch.float32, device=net.device)
    if steps < 2:
        return rows
    if kind == 'local_condition':
        for j, u in enumerate(items):
            k = int(n[u]) - 1
            if k:
                rows[j, 1:1 + k] = _device(net, cond[u][:k])
        return rows
    # frames: the round's items as one zero-padded batch through the model's
    # upsampler (a row's bits depend on its own frame, its slot and the
    # weights; a context convolution sees zeros behind an item's frames, as
    # it does for the item alone)
    F = max([-(-steps // net.lc_hop)] + [int(cond[u].shape[0]) for u in items])
    fr = torch.zeros((B, F, Lc), dtype=torch.float32, device=net.device)
    for j, u in enumerate(items):
        fr[j, :int(cond[u].shape[0])] = _device(net, cond[u])
    up = net.upsample_local_condition(fr, steps)
    left = torch.zeros(B, dtype=torch.int64)
    left[:len(items)] = torch.from_numpy(n[items] - 1)
    keep = torch.arange(steps - 1)[None, :] < left[:, None]
    rows[:, 1:] = torch.where(keep.to(net.device)[:, :, None],
                              up[:, :steps - 1], rows[:, 1:])
    return rows


def synthesize(net, lengths, *, seeds, batch=32, first_samples=None,
               global_condition=None, local_condition=None, frames=None,
               temperature=1.0, top_k=None, top_p=None,
               max_round_bytes=16 << 30, schedule='rounds', quantum=None):
    """Generate item u's n_u = lengths[u] samples behind its first (given)
    code first_samples[u] (default Q // 2), drawing with seeds[u], for every
    item, in the rounds of plan_rounds(lengths, batch).  Returns
    Synthesis(codes, rounds, steps, occupancy): codes[u] a device int32
    [n_u], without the first code (module docstring: the contract).

    global_condition: None, one id, or one id per item.  local_condition (a
    repetition-row LC model): a list of [>= n_u, Lc] rows at audio rate, row
    k beside generated sample k; frames (a model built with
    local_condition_upsample_scales): a list of [F_u, Lc] with F_u >=
    ceil(n_u / hop), upsampled by the model.  Exactly one of the two where
    the model has LC, neither where it has none.  A round whose rows
    [B, steps, Lc] exceed max_round_bytes is refused.

    schedule: 'rounds' (above), or 'queue': the restart queue of plan_queue,
    in which a slot whose item has ended takes the next item at once instead
    of idling to the end of a round.  The batched generator runs one
    segment of lock-step steps between consecutive admission times; at each
    of them the admitted slots are restarted (continue_generation_batch's
    `restart`).  quantum: admission times are multiples of it; None: max(1,
    net.fastgen_graph_steps // 10), so that every segment but the last is a
    whole number of the short captured graph.  The codes are the same bits
    for either schedule and any quantum (the contract); `rounds` of the
    result stays plan_rounds(...).rounds (callers group ragged batches by
    it), `steps` and `occupancy` are those of the schedule that ran, and
    max_round_bytes applies to the rows of the longest segment.

    Every argument is checked before the library or a device is touched;
    nothing waits for the device beyond what generate_batch waits for.  The
    last, partial round is padded to `batch` streams (seed 0, zero rows), so
    that every round runs on the same generator state."""
    n = _ints(lengths, 'synthesize: lengths', 1)
    if n.size < 1:
        raise ValueError('synthesize: lengths must name at least one item')
    U = n.size
    B = _batch(batch)
    sd = [int(v) for v in seeds]
    if len(sd) != U:
        raise ValueError('synthesize: %d seeds for %d items (one draw seed '
                         'per item)' % (len(sd), U))
    Q = int(net.Q)
    if first_samples is None:
        first = np.full(U, Q // 2, np.int64)
    else:
        first = _ints(first_samples, 'synthesize: first_samples')
        if first.shape != (U,) or (first < 0).any() or (first >= Q).any():
            raise ValueError('synthesize: first_samples must be %d codes in '
                             '[0, %d)' % (U, Q))
    gc = None
    if global_condition is not None:
        gc = _ints(np.asarray(global_condition).reshape(-1),
                   'synthesize: global_condition')
        if gc.size == 1:
            gc = np.repeat(gc, U)
        if gc.size != U:
            raise ValueError('synthesize: global_condition has %d ids for %d '
                             'items' % (gc.size, U))
    kind, cond = _check_lc(net, n, local_condition, frames)
    sampling.check(top_k, top_p)
    if not (np.isfinite(float(temperature)) and float(temperature) > 0.0):
        raise ValueError('synthesize: temperature must be a positive finite '
                         'number, got %r' % (temperature,))
    if schedule not in SCHEDULES:
        raise ValueError('synthesize: schedule must be one of %s, got %r'
                         % (', '.join(SCHEDULES), schedule))
    if quantum is not None:
        quantum = _quantum(quantum)
    plan = plan_rounds(n, B)
    if schedule == 'queue':
        if quantum is None:
            quantum = max(1, int(net.fastgen_graph_steps) // 10)
        qplan = plan_queue(n, B, quantum)
        codes = _run_queue(net, n, qplan, min(B, U), sd, first, gc, kind,
                           cond, int(max_round_bytes),
                           dict(temperature=temperature, top_k=top_k,
                                top_p=top_p))
        return Synthesis(codes, plan.rounds, qplan.steps, qplan.occupancy)
    # one round: its own size; else every round runs `batch` streams
    Br = B if len(plan.rounds) > 1 else len(plan.rounds[0])
    if kind is not None:
        need = Br * int(n[plan.rounds[0][0]]) * net.Lc * 4
        if need > int(max_round_bytes):
            raise ValueError(
                'synthesize: the local-conditioning rows of a round, [%d, '
                '%d, %d] float32 = %d bytes, exceed max_round_bytes = %d; '
                'use a smaller batch' % (Br, int(n[plan.rounds[0][0]]),
                                         net.Lc, need, int(max_round_bytes)))
    _lib.load()
    _lib.require_gpu()
    codes = [None] * U
    for items in plan.rounds:
        steps = int(n[items[0]])
        pad = Br - len(items)
        rows = None if kind is None else \
            _round_rows(net, kind, cond, items, n, Br, steps)
        out = net.generate_batch(
            steps, [sd[u] for u in items] + [0] * pad,
            seed_samples=np.concatenate(
                [first[items], np.full(pad, Q // 2, np.int64)])[:, None],
            temperature=temperature,
            global_condition=None if gc is None else np.concatenate(
                [gc[items], np.repeat(gc[items[:1]], pad)]),
            local_condition=rows, top_k=top_k, top_p=top_p)
        for j, u in enumerate(items):
            codes[u] = out[j, 1:1 + int(n[u])]
    return Synthesis(codes, plan.rounds, plan.steps, plan.occupancy)


def _run_queue(net, n, qplan, Bq, sd, first, gc, kind, cond, max_bytes, draw):
    """The restart queue on Bq = min(batch, items) streams -> codes.  One
    generate_batch for the first segment (its items start at 0), then one
    continue_generation_batch(restart=admitted) per segment; every call is
    given the longest segment as reserve_steps, so that all segments share
    their buffers and captured graphs.  Nothing here waits for the device:
    the last codes of a segment go to the next one as a device tensor."""
    import torch
    U, Q = n.size, int(net.Q)
    longest = max(m for _, m in qplan.segments)
    if kind is not None and Bq * longest * net.Lc * 4 > max_bytes:
        raise ValueError(
            'synthesize: the local-conditioning rows of a segment, [%d, %d, '
            '%d] float32 = %d bytes, exceed max_round_bytes = %d; use a '
            'smaller batch' % (Bq, longest, net.Lc,
                               Bq * longest * net.Lc * 4, max_bytes))
    _lib.load()
    _lib.require_gpu()
    by_start = {}
    for u in range(U):
        by_start.setdefault(qplan.start[u], []).append(u)
    cur = [None] * Bq              # the item a slot holds (or held last)
    rows = [None] * Bq             # its rows [n_u - 1, Lc] while it is live
    pieces = [[] for _ in range(U)]
    out = None
    for a, m in qplan.segments:
        # the codes of the segment before are taken out of `out` by
        # slicing only (it is never written), so a finished item keeps its
        # last code although the next item's first code takes its place
        # in the generator's sample cell
        admitted = sorted(by_start.get(a, []), key=lambda u: qplan.slot[u])
        for s in range(Bq):        # items that have ended hold no rows
            if cur[s] is not None and \
                    qplan.start[cur[s]] + int(n[cur[s]]) <= a:
                rows[s] = None
        for u in admitted:
            s = qplan.slot[u]
            cur[s] = u
            if kind is not None and n[u] > 1:
                k = int(n[u]) - 1
                # (frames: the item alone through the model's upsampler,
                # the contract's own definition of its rows)
                r = _device(net, cond[u][:k]) if kind == 'local_condition' \
                    else net.upsample_local_condition(cond[u], int(n[u]))[:k]
                rows[s] = r.contiguous()
        slots = [qplan.slot[u] for u in admitted]
        kw = dict(draw, reserve_steps=longest)
        if gc is not None:
            kw['global_condition'] = gc[cur]
        if kind is not None:
            kw['local_condition'] = net.batch_local_condition(
                [None if rows[s] is None else (rows[s], qplan.start[cur[s]])
                 for s in range(Bq)], a, m)
        seeds = [sd[u] for u in cur]
        if a == 0:
            out = net.generate_batch(m, seeds,
                                     seed_samples=first[cur][:, None],
                                     **kw)[:, 1:]
        else:
            last = out[:, -1]
            if slots:
                last = last.index_copy(
                    0, torch.tensor(slots, dtype=torch.int64
                                    ).to(last.device),
                    torch.from_numpy(first[admitted].astype(np.int32)
                                     ).to(last.device))
            out = net.continue_generation_batch(m, last, seeds,
                                                restart=slots or None, **kw)
        for s in range(Bq):
            u = cur[s]
            lo = max(a, qplan.start[u]) - a
            hi = min(a + m, qplan.start[u] + int(n[u])) - a
            if hi > lo:
                pieces[u].append(out[s, lo:hi])
    return [p[0] if len(p) == 1 else torch.cat(p) for p in pieces]


def copy_synthesize(net, spec, audios, *, seeds, batch=32,
                    global_condition=None, temperature=1.0, top_k=None,
                    top_p=None, schedule='rounds', quantum=None):
    """Copy synthesis of many utterances: every utterance's conditioning is
    computed from its own audio (float [n_u]) by the log-mel front end `spec`
    (net.local_condition_from_audio: frames for an upsampler model, rows for
    a repetition-row model, which then holds the rows of ALL utterances on
    the device at once), then `synthesize` generates n_u samples per
    utterance.  Returns (Synthesis, waves): waves[u] the decoded audio,
    device float32 [n_u].  No host wait beyond synthesize's."""
    from . import features
    from .ops import mu_law_decode
    if not features.is_spec(spec):
        raise ValueError('copy_synthesize: spec must be a MelSpec or a '
                         'frontend.MelPitchSpec')
    if not net.Lc:
        raise ValueError('copy_synthesize: this model was built without '
                         'local conditioning')
    audios = [np.asarray(a, np.float32).reshape(-1) for a in audios]
    if not audios or min(a.shape[0] for a in audios) < 1:
        raise ValueError('copy_synthesize: every utterance needs at least '
                         'one sample')
    cond = [net.local_condition_from_audio(spec, a) for a in audios]
    syn = synthesize(net, [a.shape[0] for a in audios], seeds=seeds,
                     batch=batch, global_condition=global_condition,
                     temperature=temperature, top_k=top_k, top_p=top_p,
                     schedule=schedule, quantum=quantum,
                     **{'frames' if net.lc_up else 'local_condition': cond})
    return syn, [mu_law_decode(c, net.Q) for c in syn.codes]


def deemphasize(emphasis, waves, groups):
    """waves[u] (device float32 [n_u], the decoded output of a model trained
    on the pre-emphasised signal) through the inverse filter on the device
    (emphasis.Emphasis.de), one ragged batch with `lengths` per group of
    utterances (`groups`: lists of indices, e.g. Synthesis.rounds).  Returns
    the new list; no host wait."""
    out = list(waves)
    for items in groups:
        for u, w in zip(items, emphasis.de_ragged([waves[u] for u in items])):
            out[u] = w
    return out


def lpc_coefficients(lp, audios):
    """The predictor coefficients (lpc.LinearPrediction `lp`) of every
    utterance's natural original audios[u], float [n_u]: device float32
    [ceil(n_u / hop), order] each, from the raw log-mel frames of the
    utterance alone -- the frames that also condition it.  No host wait."""
    return [lp.coefficients_of(np.asarray(a, np.float32).reshape(-1))
            for a in audios]


def lpc_synthesize(lp, coeffs, waves, groups):
    """waves[u] (device float32 [n_u], the decoded output of a model trained
    on the linear-prediction excitation) through the all-pole filter of
    coeffs[u] (float32 [F_u, order], e.g. lpc_coefficients') on the device
    (lpc.LinearPrediction.synthesis), one ragged batch with `lengths` per
    group of utterances (`groups`: lists of indices, e.g. Synthesis.rounds).
    Returns the new list; no host wait."""
    out = list(waves)
    for items in groups:
        done = lp.synthesis_ragged([waves[u] for u in items],
                                   [coeffs[u] for u in items])
        for u, w in zip(items, done):
            out[u] = w
    return out


def _padded_groups(generated, original, groups):
    """Per group of utterances (`groups`: lists of indices): (g, o, n) --
    generated[u] and original[u], float [n_u] each, as two zero-padded device
    float32 [len(group), max n_u] batches, and their lengths, int64 numpy."""
    import torch
    device = generated[0].device
    for items in groups:
        n = np.array([int(generated[u].shape[0]) for u in items], np.int64)
        T = int(n.max())
        g = torch.zeros((len(items), T), dtype=torch.float32, device=device)
        o = torch.zeros_like(g)
        for j, u in enumerate(items):
            g[j, :n[j]] = generated[u]
            o[j, :n[j]] = torch.as_tensor(original[u], dtype=torch.float32
                                          ).to(device)
        yield g, o, n


def log_mel_distance(spec, generated, original, groups):
    """(log_mel_mae_db, log_mel_lsd_db) between the RAW log-mel features
    (`spec` without its normaliser, the tables shared) of generated[u] and
    original[u], float [n_u] each, over all utterances: features.
    frame_distance per group of utterances (`groups`: lists of indices, e.g.
    Synthesis.rounds), zero padded with `lengths` set so that padding frames
    are zeros on both sides and excluded by nframes.  One host wait, at the
    end."""
    import torch
    from . import features
    # (a mel + F0 front end compares its mel part)
    raw = spec.with_normalizer(None) if isinstance(spec, features.MelSpec) \
        else spec.mel
    parts, nframes = [], []
    for g, o, n in _padded_groups(generated, original, groups):
        nf = -(-n // raw.hop)
        parts.append(features.frame_distance(raw(g, n), raw(o, n), nf))
        nframes.append(nf)
    total = features.FrameDistance(*(torch.cat(t) for t in zip(*parts)))
    return total.summary(np.concatenate(nframes), raw.n_mels)


def pitch_distance(tracker, generated, original, groups):
    """The F0 error of generated[u] against original[u], float [n_u] each,
    over all utterances: both tracked by `tracker` (a pitch.PitchTracker, a
    pitch.PitchPath, or any callable (audio, lengths) -> Pitch with a `hop`) in
    the zero-padded groups of log_mel_distance with `lengths` set, compared
    by pitch.f0_error over each utterance's real frames.  Returns
    F0Error.summary(): f0_rmse_cents, gross_pitch_error, vuv_error,
    voiced_frames (of the originals), frames.  One host wait, at the end."""
    import torch
    from . import pitch
    parts = []
    for g, o, n in _padded_groups(generated, original, groups):
        parts.append(pitch.f0_error(tracker(g, n), tracker(o, n),
                                    -(-n // tracker.hop)))
    return pitch.F0Error(*(torch.cat(t) for t in zip(*parts))).summary()


def stft_distance(dist, generated, original, groups):
    """The multi-resolution STFT distance (`dist`: a spectral.StftDistance) of
    generated[u] against original[u], float [n_u] each, over all utterances,
    in the zero-padded groups of log_mel_distance with `lengths` set.  A
    clip's sums do not depend on its group.  Returns StftSums.summary() over
    the utterances in the order of `groups`.  One host wait, at the end."""
    from . import spectral
    parts, lengths = [], []
    for g, o, n in _padded_groups(generated, original, groups):
        parts.append(dist(g, o, n))
        lengths.append(n)
    return spectral.StftSums.cat(parts).summary(np.concatenate(lengths))


def stoi(meter, generated, original, groups):
    """STOI and ESTOI (`meter`: a stoi.Stoi at the utterances' sample rate) of
    generated[u] against original[u], float [n_u] each, over all utterances,
    in the zero-padded groups of log_mel_distance with `lengths` set.  A
    clip's sums do not depend on its group.  Returns StoiSums.summary() over
    the utterances in the order of `groups`.  One host wait, at the end."""
    from . import stoi as stoi_
    return stoi_.StoiSums.cat(
        [meter(g, o, n) for g, o, n in
         _padded_groups(generated, original, groups)]).summary()


def mel_cepstral_distortion(spec, generated, original, groups, order=13):
    """The mel-cepstral distortion in dB (spectral.mcd_db: DCT-II of the RAW
    log-mel features, the spec log_mel_distance picks, coefficients 1 ..
    order) of generated[u] against original[u] over all utterances, in the
    same groups.  Returns {'mcd_db', 'order', 'n_mels', 'frames'}.  One host
    wait, at the end."""
    import torch
    from . import features, spectral
    raw = spec.with_normalizer(None) if isinstance(spec, features.MelSpec) \
        else spec.mel
    parts, nframes = [], []
    for g, o, n in _padded_groups(generated, original, groups):
        nf = -(-n // raw.hop)
        parts.append(spectral.cepstral_distance(raw(g, n), raw(o, n), nf,
                                                order))
        nframes.append(nf)
    nframes = np.concatenate(nframes)
    return {'mcd_db': spectral.mcd_db(torch.cat(parts), nframes),
            'order': int(order), 'n_mels': raw.n_mels,
            'frames': int(nframes.sum())}


def griffin_lim_baseline(gl, spec, original, groups):
    """The Griffin-Lim reconstructions (`gl`: a griffin_lim.GriffinLim over
    the RAW front end of `spec`, the spec log_mel_distance picks) of
    original[u], float [n_u] each: per group of utterances (`groups`: lists of
    indices) the raw log-mel features of the zero-padded originals
    (wn_melspec, `lengths` set) go through `gl`, utterance u drawing its
    phases with key u, so that its waveform does not depend on the grouping.
    Returns the waves, device float32 [n_u] each, in the order of `original`:
    what the distance helpers take as `generated`.  No host wait."""
    import torch
    from . import _lib, features
    raw = spec.with_normalizer(None) if isinstance(spec, features.MelSpec) \
        else spec.mel
    if gl.spec.with_normalizer(None).settings() != raw.settings():
        raise ValueError('griffin_lim_baseline: gl was built over another '
                         'front end than the spec\'s')
    _lib.load()
    _lib.require_gpu()
    device = torch.device('cuda', torch.cuda.current_device())
    dev = [torch.as_tensor(o, dtype=torch.float32).to(device) for o in original]
    out = [None] * len(original)
    # (the zero-padded groups of the distance helpers, the originals on both
    # sides)
    for items, (o, _, n) in zip(groups, _padded_groups(dev, original, groups)):
        x = gl(raw(o, n), lengths=n, keys=list(items))
        for j, u in enumerate(items):
            out[u] = x[j, :n[j]]
    return out


def write_wavs(waves, names, directory, sample_rate):
    """waves[u] (device float32 [n_u]) -> directory/<names[u]>.wav, float32
    as generate.py writes them.  Returns the paths."""
    import os
    from scipy.io import wavfile
    os.makedirs(directory, exist_ok=True)
    paths = []
    for w, name in zip(waves, names):
        paths.append(os.path.join(directory, name + '.wav'))
        wavfile.write(paths[-1], int(sample_rate),
                      w.detach().cpu().numpy().astype(np.float32))
    return paths
