"""Held-out evaluation, host side: one deterministic pass over a directory of
validation clips (ValidationSet), their WaveNetModel.score results summed on
the device (totals / evaluate), evaluation under another parameter vector such
as the optimizer's EMA shadow (parameters_swapped) and the sum over
data-parallel ranks (sum_over_ranks).  train.py --validation_dir and the
top-level evaluate.py drive it."""
import contextlib
import math

import numpy as np
import torch

from . import audio_reader as ar


class ValidationSet(object):
    """The clips of `directory` as the training reader would prepare them --
    the same loading, silence trimming and feature alignment, through
    audio_reader's own functions -- in ONE deterministic pass: files in
    sorted order (rank's shard files[rank::world]), no shuffling, no threads.
    Pieces are cut per file (sample_size samples each, the last one shorter);
    nothing is carried from one file into the next.  With sample_size None
    the pieces are whole utterances, sorted by length (ties in file order)
    so that batches pad little.

    Local conditioning as AudioReader: `<clip>.npy` [frames, lc_channels]
    next to every wav, upsampled by repetition (lc_hop samples per frame), or
    with lc_frames=True the clip's frames and the piece's offset.  Global
    conditioning: the id of `p<id>_<rec>.wav` (below gc_cardinality where
    that is given).

    history=H > 0: piece k of a file brings h = min(H, k * sample_size)
    samples of its left context, [k * sample_size - h, (k + 1) * sample_size)
    of the file, with the conditioning of those samples; net.score gets
    history=h and counts only the piece's own rows (`piece_history`: h per
    piece)."""

    def __init__(self, directory, sample_rate, *, sample_size=None,
                 silence_threshold=None, gc_enabled=False, gc_cardinality=None,
                 lc_channels=None, lc_hop=None, lc_frames=False, rank=0,
                 world=1, history=0):
        if isinstance(history, bool) or \
                not isinstance(history, (int, np.integer)) or history < 0:
            raise ValueError('history must be a non-negative int, got %r'
                             % (history,))
        self.history = int(history)
        self.piece_history = []
        self.lc_channels = lc_channels
        self.lc_frames = bool(lc_frames) and lc_channels is not None
        self.gc_enabled = bool(gc_enabled)
        if lc_channels is not None and not lc_hop:
            raise ValueError('local conditioning needs lc_hop (samples per '
                             'feature frame)')
        if sample_size is not None and int(sample_size) < 1:
            raise ValueError('sample_size must be positive, got %r'
                             % (sample_size,))
        files = ar.find_files(directory)
        if not files:
            raise ValueError("No audio files found in '{}'.".format(directory))
        if self.gc_enabled and ar.not_all_have_id(files):
            raise ValueError("Global conditioning is enabled, but file names "
                             "do not conform to pattern having id.")
        self.files = files[rank::world]
        # (audio [n], file, gc id or None, rows [n, Lc] | (frames, offset) |
        # None)
        self.pieces = []
        for f in self.files:
            gc = ar.category_id_of(f) if self.gc_enabled else None
            if gc is not None and gc_cardinality is not None and \
                    not 0 <= gc < gc_cardinality:
                raise ValueError('%s: speaker id %d outside the model\'s '
                                 'gc_cardinality %d' % (f, gc, gc_cardinality))
            audio = ar.load_wav(f, sample_rate)
            lc, lo = None, 0
            if self.lc_frames:
                lc = ar.pad_lc_frames(np.load(ar.lc_path_of(f)), lc_hop,
                                      audio.shape[0], lc_channels)
                if silence_threshold is not None:
                    lo, hi = ar.trim_bounds(audio, silence_threshold)
                    audio = audio[lo:hi]
            else:
                if lc_channels is not None:
                    lc = ar.load_lc(ar.lc_path_of(f), lc_hop, audio.shape[0],
                                    lc_channels)
                if silence_threshold is not None:
                    if lc is not None:
                        audio, lc = ar.trim_silence_lc(audio, lc,
                                                       silence_threshold)
                    else:
                        audio = ar.trim_silence(audio, silence_threshold)
            step = int(sample_size) if sample_size else max(audio.size, 1)
            for k in range(0, audio.size, step):
                h = min(self.history, k)
                piece = np.ascontiguousarray(audio[k - h:k + step])
                if self.lc_frames:
                    cond = (lc, int(lo) + k - h)
                else:
                    cond = None if lc is None else lc[k - h:k + step]
                self.pieces.append((piece, f, gc, cond))
                self.piece_history.append(h)
        if not sample_size:
            # (whole utterances: every h above is 0)
            self.pieces.sort(key=lambda p: p[0].shape[0])   # (stable)

    def __len__(self):
        return len(self.pieces)

    def batches(self, B):
        """Yields (audio float32 [b, Tmax], lengths int64 [b], gc ids int32
        [b] or None, lc) with b <= B pieces in order, zero padded behind
        each piece; lc: rows float32 [b, Tmax, Lc], or (frames float32
        [b, Fmax, Lc], offsets int64 [b]) in frames mode, or None.  A set
        built with history > 0 yields a fifth item, the pieces' history
        int64 [b] (counted in lengths)."""
        B = int(B)
        if B < 1:
            raise ValueError('batch size must be positive, got %d' % B)
        for i in range(0, len(self.pieces), B):
            group = self.pieces[i:i + B]
            b = len(group)
            lengths = np.array([p[0].shape[0] for p in group], np.int64)
            tmax = int(lengths.max())
            audio = np.zeros((b, tmax), np.float32)
            for j, p in enumerate(group):
                audio[j, :lengths[j]] = p[0]
            gc = np.array([p[2] for p in group], np.int32) \
                if self.gc_enabled else None
            lc = None
            if self.lc_frames:
                fmax = max(p[3][0].shape[0] for p in group)
                fr = np.zeros((b, fmax, self.lc_channels), np.float32)
                for j, p in enumerate(group):
                    fr[j, :p[3][0].shape[0]] = p[3][0]
                lc = (fr, np.array([p[3][1] for p in group], np.int64))
            elif self.lc_channels is not None:
                lc = np.zeros((b, tmax, self.lc_channels), np.float32)
                for j, p in enumerate(group):
                    lc[j, :lengths[j]] = p[3]
            if self.history > 0:
                yield audio, lengths, gc, lc, np.array(
                    self.piece_history[i:i + B], np.int64)
            else:
                yield audio, lengths, gc, lc


def with_features(net, spec, batches):
    """`batches` of an audio-only ValidationSet with the local conditioning
    computed on the device from each batch's own audio (features.MelSpec
    `spec`): frames at offset 0 for an upsampler model, else rows."""
    for audio, lengths, gc, _, *hist in batches:
        lc = net.local_condition_from_audio(spec, audio, lengths)
        yield (audio, lengths, gc, ((lc, 0) if net.lc_up else lc), *hist)


def with_emphasis(emphasis, batches):
    """`batches` with the audio pre-emphasised on the device (emphasis.
    Emphasis), each clip over its own length -- behind with_features, whose
    features are those of the natural signal."""
    for audio, lengths, gc, lc, *hist in batches:
        yield (emphasis.pre(audio, lengths), lengths, gc, lc, *hist)


def with_lpc(lp, spec, batches):
    """`batches` with the audio replaced by its linear-prediction excitation
    on the device (lpc.LinearPrediction `lp`; the coefficients from each
    clip's own raw log-mel, each clip over its own length) -- behind
    with_features, whose features are those of the natural signal.  `spec`:
    the front end those features came from; its raw mel part must be lp's
    (a ValueError here, before any batch is taken)."""
    from . import features
    raw = spec.with_normalizer(None) if isinstance(spec, features.MelSpec) \
        else spec.mel
    if raw.settings() != lp.spec.with_normalizer(None).settings():
        raise ValueError('with_lpc: lp was built over another front end than '
                         'the features\' (%r, %r)'
                         % (lp.spec.with_normalizer(None).settings(),
                            raw.settings()))

    def excited():
        for audio, lengths, gc, lc, *hist in batches:
            cf = lp.coefficients_of(audio, lengths)
            yield (lp.analysis(audio, cf, lengths), lengths, gc, lc, *hist)
    return excited()


def totals(net, batches, max_batches=None, *, input_noise=None, rank=0,
           world=1):
    """float64 [4] on the device: (sum of nll, targets, hits, clips) over
    net.score of every batch (at most max_batches of them).  No host wait.
    input_noise (input_noise.InputNoise): the network reads perturbed codes,
    the targets stay clean; the key of a clip is its running index in this
    pass times `world` plus `rank`."""
    tot, clips = None, 0
    for i, (audio, lengths, gc, lc, *hist) in enumerate(batches):
        if max_batches is not None and i >= max_batches:
            break
        off = 0
        if isinstance(lc, tuple):
            lc, off = lc
        # (a fifth item: the pieces' history, ValidationSet(history=...))
        kw = dict(history=hist[0]) if hist else {}
        if input_noise is not None:
            b = int(np.shape(lengths)[0])
            kw.update(input_noise=input_noise, noise_keys=(
                clips + np.arange(b, dtype=np.int64)) * world + rank)
        s = net.score(audio, gc, local_condition_batch=lc,
                      local_condition_offset=off, lengths=lengths, **kw)
        # (a mixture-of-logistics head has no arg-max: its hits are NaN and
        # summary reports no accuracy)
        hits = s.correct.sum().to(torch.float64) if s.correct is not None \
            else torch.full((), float('nan'), dtype=torch.float64,
                            device=s.nll.device)
        part = torch.stack([s.nll.sum(), s.count.sum().to(torch.float64),
                            hits])
        tot = part if tot is None else tot + part
        clips += int(np.shape(lengths)[0])
    if tot is None:
        tot = torch.zeros(3, dtype=torch.float64, device=net.device)
    return torch.cat([tot, torch.tensor([float(clips)], dtype=torch.float64,
                                        device=tot.device)])


def summary(tot):
    """The dict of `evaluate` from totals() (waits for the device here)."""
    nll, count, correct, clips = (float(x) for x in tot.detach().cpu())
    nats = nll / count if count else float('nan')
    return {'nll_per_sample': nats,
            'bits_per_sample': nats / math.log(2.0),
            'accuracy': None if correct != correct else
            correct / count if count else float('nan'),
            'samples': int(count), 'clips': int(clips)}


def evaluate(net, batches, max_batches=None, **noise):
    """Score `batches` (ValidationSet.batches items) with net.score, the
    sums kept in float64 on the device and fetched once at the end.  Returns
    nll_per_sample (nats per predicted sample), bits_per_sample (that
    / ln 2), accuracy (top-1), samples (predicted samples) and clips.
    noise: totals' input_noise, rank and world."""
    return summary(totals(net, batches, max_batches, **noise))


@contextlib.contextmanager
def parameters_swapped(net, flat):
    """Evaluate with another flat parameter vector laid out like net.params
    (the optimizer's EMA shadow): inside the block the model computes with
    `flat`; its own parameters are back afterwards, also after an exception.

    The values are copied INTO net.params, whose address recorded launch
    plans hold and key on: the plans stay valid.  Every image a pass derives
    from the parameters (packed stack weights, the fused skip image,
    transposes, bf16 splits) is rebuilt by that pass, and the optimizers'
    updates invalidate nothing for that reason; load_state_dict drops the
    fast-generation states, which hold packed weights.  So does this, on
    entry and on exit."""
    flat = torch.as_tensor(flat)
    if flat.numel() != net.params.numel():
        raise ValueError('parameters_swapped: %d floats for a model of %d'
                         % (flat.numel(), net.params.numel()))
    saved = net.params.detach().clone()

    def put(values):
        with torch.no_grad():
            net.params.copy_(values.reshape(-1))
        net._gen = None
        net._bgen = None
    put(flat.detach())
    try:
        yield net
    finally:
        put(saved)


def sum_over_ranks(totals_, device=None):
    """One all_reduce(SUM) of a small float64 tensor over the default group
    (returned on the tensor's own device); the identity when
    torch.distributed is not initialised."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return totals_
    t = totals_.detach().to(dtype=torch.float64,
                            device=device if device is not None
                            else totals_.device).clone()
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t.to(totals_.device)
