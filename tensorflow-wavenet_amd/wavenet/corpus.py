"""Device-resident training corpus: the whole (trimmed) corpus lives in one
device buffer and every batch is cut from it by a kernel (csrc/wn_corpus.hip).
No reader thread, no queue, no host-to-device copy per step.

`CorpusIndex` is the host side: the item table and the sampling rule, numpy
only.  `DeviceCorpus` loads the files once with the reader's own functions,
keeps them on the device and hands out batches.

The rule (tests/corpus_ref.py restates it independently):

    items    crop 'pieces': utterance u of n_u samples gives the pieces
             [k size, min((k + 1) size, n_u)) (the reader's cut; without
             sample_size the whole utterance is one item);
             crop 'random': one item per utterance, a window of
             min(size, n_u) samples drawn afresh at every visit
    slot     g = step * B + j, j < B;  epoch e = g // P;  P = len(items)
    item     perm_e[g % P];  perm_e = the item indices sorted by the key
             draw_bits(seed, e * P + i), ascending, ties by i
    start    'random', n_u > size:
             draw_bits(seed ^ 0x63726f70, g) % (n_u - size + 1)
    draw_bits(seed, c) = splitmix64(seed ^ splitmix64(c))   (csrc/wn_common.h)
    history  H > 0 (default 0): h = min(H, start), start' = start - h,
             n' = n + h -- the piece with h samples of its true left context
             in front, which the loss feeds but does not predict
             (WaveNetModel.loss, history=).  Everything below uses
             (start', n').  Items, orders and drawn starts do not depend on H.

The order is a pure function of (seed, step, B): a run resumed at step k
continues the uninterrupted run's sequence, and a batch may straddle epochs.
Data-parallel ranks shard the sorted files like the reader, files[rank::world],
each with its own index over its shard and the same seed.

Frames (utterance-context local conditioning, hop samples per frame, frame f
beside samples f * hop .. f * hop + hop - 1, m = WaveNetModel.LC_CONTEXT_MAX):

    f_lo   = max(0, start // hop - m)
    f_hi   = min(F_u, (start + n - 1) // hop + 1 + m)
    offset = start - f_lo * hop
    Fw     = (T + hop - 2) // hop + 1 + 2 m       (window_frames: any start)

Normalised frames (normalize=): 'corpus' sums x and x * x per channel over
the resident raw frames with one wn_feature_stats launch (features.
FeatureStats: float64, one fixed order), over all ranks' shards through
`stats_allreduce`, builds features.Normalizer.from_stats from them and
normalises the resident frames in place, once; the gathers then copy
normalised frames.  A features.Normalizer is applied the same way.

loss(..., local_condition_batch=frames, local_condition_offset=offset) then
selects what it would select from the whole utterance's frames at offset =
start, the frame-context convolution's neighbours and its zeros at the true
utterance edges included.
"""
import collections

import numpy as np

from . import _lib

CROP_SALT = 0x63726f70          # 'crop'
LC_CONTEXT_MAX = 8              # WaveNetModel.LC_CONTEXT_MAX
_M64 = (1 << 64) - 1

Plan = collections.namedtuple('Plan', 'utt start n gc T history')
Batch = collections.namedtuple('Batch',
                               'audio lengths gc frames offsets rows history')


def _is_int(v):
    return isinstance(v, (int, np.integer)) and \
        not isinstance(v, (bool, np.bool_))


def splitmix64(x):
    """splitmix64 of csrc/wn_common.h on uint64 arrays (wrapping)."""
    x = np.asarray(x, np.uint64)
    with np.errstate(over='ignore'):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def draw_bits(seed, counter):
    """draw_bits of csrc/wn_common.h: uint64 array of the counters' bits."""
    return splitmix64(np.uint64(int(seed) & _M64) ^ splitmix64(counter))


def window_frames(T, hop, m=LC_CONTEXT_MAX):
    """Fw: frames a window of T samples needs at most, whatever its start
    (wn_corpus_window_frames)."""
    return (int(T) + int(hop) - 2) // int(hop) + 1 + 2 * int(m)


class CorpusIndex(object):
    """The item table and the sampling rule of a corpus of utterances with
    `lengths` samples (module docstring).  Host only: numpy, no device, no
    library."""

    def __init__(self, lengths, category_ids=None, sample_size=None,
                 crop='pieces', seed=0, history=0):
        if crop not in ('pieces', 'random'):
            raise ValueError("crop must be 'pieces' or 'random', got %r"
                             % (crop,))
        if sample_size is not None and \
                (not _is_int(sample_size) or sample_size < 1):
            raise ValueError('sample_size must be a positive int or None, '
                             'got %r' % (sample_size,))
        if crop == 'random' and sample_size is None:
            raise ValueError("crop 'random' needs sample_size")
        if not _is_int(seed) or not 0 <= seed <= _M64:
            raise ValueError('seed must be an int in [0, 2^64), got %r'
                             % (seed,))
        if not _is_int(history) or not 0 <= history < 1 << 31:
            raise ValueError('history must be an int in [0, 2^31), got %r'
                             % (history,))
        self.history = int(history)
        n = np.asarray(lengths)
        if n.size == 0:
            n = n.astype(np.int64).reshape(-1)
        if n.ndim != 1 or n.dtype == np.bool_ or \
                not np.issubdtype(n.dtype, np.integer) or (n < 0).any() or \
                (n >= 1 << 31).any():
            raise ValueError('lengths must be non-negative ints below 2^31 '
                             '[utterances]')
        self.lengths = n.astype(np.int64)
        self.category_ids = None
        if category_ids is not None:
            c = np.asarray(category_ids)
            if c.shape != n.shape or c.dtype == np.bool_ or \
                    not np.issubdtype(c.dtype, np.integer):
                raise ValueError('category_ids must be %d ints' % n.shape[0])
            self.category_ids = c.astype(np.int32)
        self.sample_size = None if sample_size is None else int(sample_size)
        self.crop, self.seed = crop, int(seed)
        # flat offsets of the utterances in the concatenation
        self.offsets = np.concatenate([[0], np.cumsum(self.lengths)[:-1]]) \
            .astype(np.int64) if n.size else np.zeros(0, np.int64)
        utt, start = [], []
        for u, nu in enumerate(self.lengths.tolist()):
            if nu == 0:
                continue            # (trimmed to nothing: no item)
            if crop == 'pieces' and self.sample_size:
                ks = range(0, nu, self.sample_size)
                utt.extend([u] * len(ks))
                start.extend(ks)
            else:
                utt.append(u)
                start.append(0)
        self.item_utt = np.asarray(utt, np.int32)
        self.item_start = np.asarray(start, np.int32)
        self.P = int(self.item_utt.shape[0])
        if self.P == 0:
            raise ValueError('the corpus has no items: no utterance holds a '
                             'sample')
        self._perms = {}

    def __len__(self):
        return self.P

    @property
    def items(self):
        """int64 [P, 2]: (utterance, start of the piece within it; 0 for a
        whole utterance and for a random window, whose start is drawn)."""
        return np.stack([self.item_utt, self.item_start], 1).astype(np.int64)

    def perm(self, e):
        """Epoch e's order: int32 [P]."""
        e = int(e)
        if e not in self._perms:
            if len(self._perms) > 4:
                self._perms.clear()
            c0 = (e * self.P) & _M64
            keys = draw_bits(self.seed, np.uint64(c0) +
                             np.arange(self.P, dtype=np.uint64))
            self._perms[e] = np.argsort(keys, kind='stable').astype(np.int32)
        return self._perms[e]

    def epoch_of(self, step, B):
        """Epoch of the first slot of batch `step`."""
        return (int(step) * int(B)) // self.P

    def epochs(self, step, B):
        """(first epoch, number of epochs) batch `step` touches."""
        g0 = int(step) * int(B)
        e0 = g0 // self.P
        return e0, (g0 + int(B) - 1) // self.P - e0 + 1

    def plan(self, step, B, T=None):
        """Batch `step` of B slots: Plan(utt, start, n, gc, T, history): per
        slot the utterance, the first sample within it, the sample count, the
        speaker id (None without category_ids); T = max(n); the leading
        samples of the slot that are history (0 for an index without).  A
        given T cuts n (and history to n).  With history, start and n are
        start' and n' of the module docstring."""
        if not _is_int(step) or step < 0 or not _is_int(B) or B < 1:
            raise ValueError('plan: step >= 0 and B >= 1 are required, got '
                             '%r, %r' % (step, B))
        if T is not None and (not _is_int(T) or T < 1):
            raise ValueError('plan: T must be a positive int, got %r' % (T,))
        g = int(step) * int(B) + np.arange(int(B), dtype=np.int64)
        e, r = g // self.P, g % self.P
        item = np.empty(int(B), np.int64)
        for ee in np.unique(e):
            item[e == ee] = self.perm(ee)[r[e == ee]]
        utt = self.item_utt[item].astype(np.int64)
        nu = self.lengths[utt]
        if self.crop == 'random':
            size = self.sample_size
            n = np.minimum(size, nu)
            span = np.maximum(nu - size + 1, 1).astype(np.uint64)
            bits = draw_bits(self.seed ^ CROP_SALT, g.astype(np.uint64))
            start = (bits % span).astype(np.int64)
        else:
            start = self.item_start[item].astype(np.int64)
            n = nu - start if not self.sample_size else \
                np.minimum(self.sample_size, nu - start)
        h = np.minimum(self.history, start)
        start, n = start - h, n + h
        if T is not None:
            n = np.minimum(n, int(T))
        h = np.minimum(h, n)
        gc = None if self.category_ids is None else self.category_ids[utt]
        return Plan(utt, start, n.astype(np.int64), gc,
                    int(n.max()) if T is None else int(T),
                    h.astype(np.int64))

    def frame_window(self, plan, hop, frame_counts, m=LC_CONTEXT_MAX):
        """(f_lo, f_hi, offsets) int64 [B] of a plan's frames windows
        (module docstring); frame_counts: F_u per utterance."""
        hop = int(hop)
        F = np.asarray(frame_counts, np.int64)[plan.utt]
        f_lo = np.maximum(0, plan.start // hop - m)
        f_hi = np.minimum(F, (plan.start + plan.n - 1) // hop + 1 + m)
        return f_lo, f_hi, plan.start - f_lo * hop


def shard(files, rank, world):
    """The reader's data-parallel shard of the sorted files."""
    return files[rank::world] if world > 1 else list(files)


class DeviceCorpus(object):
    """The corpus on the device and its batches (module docstring).

    batch(step, B) launches the gather on torch's current stream and returns
    without waiting for the device.  Output buffers: RING = 2 sets, used in
    turn by successive batch calls; a batch's tensors are views of its set's
    buffers (one per output: audio, frames, rows), which grow to the largest
    batch seen and are never more than that: at most RING x the largest
    B * T, B * Fw * Lc and B * T * Lc floats, however many different T a run
    meets.  Batch k's tensors are rewritten by batch call k + 2, on the
    stream current then.  Two consecutive batches never share memory, and
    work queued on that stream before the rewrite (the step that consumed
    batch k) has finished reading by stream order.  A consumer on another
    stream, or one that keeps a batch longer, clones it.

    The permutations of the epochs a batch touches stay on the device; a new
    epoch's goes up once, when a batch first touches it, from pinned memory
    without waiting for the device (with B > P + 1 a batch spans more than
    two epochs and every batch brings new ones).

    Loading holds the trimmed clips on the host until they are copied, one
    by one, into the device buffer: a host peak of one corpus, a device peak
    of the corpus plus one utterance's frames."""

    RING = 2

    def __init__(self, audio_dir, sample_rate, gc_enabled, sample_size=None,
                 silence_threshold=None, crop='pieces', seed=0, rank=0,
                 world=1, spec=None, device=None, max_bytes=32 << 30, *,
                 normalize=None, normalize_clip=None, stats_allreduce=None,
                 history=0):
        from . import audio_reader as ar
        from . import features
        _check_args(sample_size, crop, seed, max_bytes, history)
        if not _is_int(rank) or not _is_int(world) or not 0 <= rank < world:
            raise ValueError('0 <= rank < world is required, got rank %r, '
                             'world %r' % (rank, world))
        if spec is not None and not features.is_spec(spec):
            raise ValueError('spec must be a features.MelSpec, a '
                             'frontend.MelPitchSpec or None')
        norm_kw = _check_normalize(normalize, normalize_clip, stats_allreduce,
                                   world, None if spec is None else
                                   spec.n_mels, spec is not None)
        files = ar.find_files(audio_dir)
        if not files:
            raise ValueError("No audio files found in '{}'.".format(audio_dir))
        if gc_enabled and ar.not_all_have_id(files):
            raise ValueError("Global conditioning is enabled, but file names "
                             "do not conform to pattern having id.")
        card = None
        if gc_enabled:
            card = ar.get_category_cardinality(files)[1] + 1
            print("Detected --gc_cardinality={}".format(card))
        files = shard(files, rank, world)
        if not files:
            raise ValueError('rank %d of %d has no audio files'
                             % (rank, world))
        clips, ids, kept, total, nframes = [], [], [], 0, 0
        for f in files:
            audio = ar.load_wav(f, sample_rate)
            if silence_threshold is not None:
                lo, hi = ar.trim_bounds(audio, silence_threshold)
                audio = audio[lo:hi]
            if audio.size == 0:
                print("Warning: {} was ignored as it contains only "
                      "silence. Consider decreasing trim_silence "
                      "threshold, or adjust volume of the audio."
                      .format(f))
                continue
            total += audio.size
            if spec is not None:
                nframes += spec.num_frames(audio.size)
            _check_bytes(total, nframes * (spec.channels if spec else 0),
                         max_bytes, 'at least %%d bytes on the device after '
                         '%d of its %d files' % (len(kept) + 1, len(files)))
            clips.append(audio)
            kept.append(f)
            ids.append(ar.category_id_of(f))
        if not clips:
            raise ValueError("every audio file in '{}' trims to nothing"
                             .format(audio_dir))
        self.files = kept
        self._setup(clips, ids if gc_enabled else None, None, None,
                    dict(sample_size=sample_size, crop=crop, seed=seed,
                         history=history),
                    spec, device, max_bytes, norm_kw)
        self.gc_category_cardinality = card

    @classmethod
    def from_arrays(cls, arrays, category_ids=None, frames=None, hop=None,
                    device=None, max_bytes=32 << 30, spec=None,
                    normalize=None, normalize_clip=None, stats_allreduce=None,
                    world=1, **index_kw):
        """The same object from float32 arrays in memory (frames: one
        [F_u, Lc] array per utterance with F_u >= ceil(n_u / hop); or spec:
        the frames are computed as from files).  normalize...: as the
        constructor's; world: the number of shards this one belongs to."""
        from . import features
        self = cls.__new__(cls)
        if spec is not None and not features.is_spec(spec):
            raise ValueError('spec must be a features.MelSpec, a '
                             'frontend.MelPitchSpec or None')
        if spec is not None and frames is not None:
            raise ValueError('from_arrays: spec and frames exclude each '
                             'other')
        if not _is_int(world) or world < 1:
            raise ValueError('from_arrays: world must be a positive int, '
                             'got %r' % (world,))
        _check_args(index_kw.get('sample_size'), index_kw.get('crop', 'pieces'),
                    index_kw.get('seed', 0), max_bytes,
                    index_kw.get('history', 0))
        clips = []
        for a in arrays:
            a = np.asarray(a)
            if a.ndim != 1 or a.dtype != np.float32:
                raise ValueError('from_arrays: every utterance must be a '
                                 'float32 array [n], got %s %s'
                                 % (a.dtype, a.shape))
            clips.append(a)
        if not clips:
            raise ValueError('from_arrays: no utterances')
        if (frames is None) != (hop is None):
            raise ValueError('from_arrays: frames and hop go together')
        if frames is not None:
            if not _is_int(hop) or hop < 1:
                raise ValueError('from_arrays: hop must be a positive int, '
                                 'got %r' % (hop,))
            frames = [np.asarray(f) for f in frames]
            if len(frames) != len(clips):
                raise ValueError('from_arrays: %d frame arrays for %d '
                                 'utterances' % (len(frames), len(clips)))
            Lc = frames[0].shape[1] if frames[0].ndim == 2 else 0
            for a, f in zip(clips, frames):
                if f.ndim != 2 or f.dtype != np.float32 or Lc < 1 or \
                        f.shape[1] != Lc or f.shape[0] < -(-a.shape[0] // hop):
                    raise ValueError(
                        'from_arrays: frames must be float32 [F_u, Lc] with '
                        'F_u >= ceil(n_u / hop), got %s %s for %d samples at '
                        'hop %d' % (f.dtype, f.shape, a.shape[0], hop))
        norm_kw = _check_normalize(
            normalize, normalize_clip, stats_allreduce, world,
            spec.n_mels if spec is not None else
            (frames[0].shape[1] if frames is not None else None),
            spec is not None or frames is not None)
        self.files = None
        self._setup(clips, category_ids, frames, hop, index_kw, spec, device,
                    max_bytes, norm_kw)
        self.gc_category_cardinality = None if category_ids is None else \
            int(np.max(category_ids)) + 1
        return self

    # ------------------------------------------------------------ internals
    def _setup(self, clips, ids, frames, hop, index_kw, spec, device,
               max_bytes, norm_kw=None):
        lengths = [int(a.shape[0]) for a in clips]
        self.index = CorpusIndex(lengths, ids, **index_kw)
        Lc = spec.channels if spec is not None else \
            (frames[0].shape[1] if frames is not None else 0)
        hop = spec.hop if spec is not None else hop
        counts = None if Lc == 0 else np.asarray(
            [spec.num_frames(n) for n in lengths] if spec is not None
            else [f.shape[0] for f in frames], np.int64)
        _check_bytes(sum(lengths), 0 if counts is None else
                     int(counts.sum()) * Lc, max_bytes)
        # everything above needs neither the library nor a device
        import torch
        from . import features
        _lib.load()
        _lib.require_gpu()
        self.device = torch.device('cuda', torch.cuda.current_device()) \
            if device is None else torch.device(device)
        self.hop, self.Lc, self.spec = hop, Lc, spec
        self.world = norm_kw['world'] if norm_kw else 1
        self.normalizer = self.feature_stats = None
        raw = spec
        if spec is not None and norm_kw and norm_kw['normalize'] is not None:
            raw = spec.with_normalizer(None)    # (normalised below, once)
        elif spec is not None:
            self.normalizer = spec.normalizer
        ix = self.index

        def dev(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

        def filled(parts, sizes):
            """One device buffer of sum(sizes) floats, the parts copied in one
            by one (each dropped from `parts` once it is there)."""
            flat = torch.empty(int(sum(sizes)), dtype=torch.float32,
                               device=self.device)
            o = 0
            for k, n in enumerate(sizes):
                flat[o:o + n].copy_(torch.from_numpy(
                    np.ascontiguousarray(parts[k]).reshape(-1)))
                parts[k] = None
                o += n
            return flat
        self.flat = filled(clips, lengths)
        self._utt_off, self._utt_len = dev(ix.offsets), \
            dev(ix.lengths.astype(np.int32))
        self._item_utt, self._item_start = dev(ix.item_utt), \
            dev(ix.item_start)
        self.frame_counts, self.frames_flat = counts, None
        if counts is not None:
            fr_off = np.concatenate([[0], np.cumsum(counts)[:-1]]) \
                .astype(np.int64)
            self._fr_off, self._fr_len = dev(fr_off), \
                dev(counts.astype(np.int32))
        mel_stats = None
        if spec is not None:
            # each utterance's log-mel frames, once (tools/make_lc_features.py
            # does the same for a whole utterance), written to their place
            self.frames_flat = torch.empty(int(counts.sum()) * Lc,
                                           dtype=torch.float32,
                                           device=self.device)
            composite = not isinstance(spec, features.MelSpec)
            if composite and raw is not spec and _wants_stats(**norm_kw):
                mel_stats = features.FeatureStats(spec.n_mels)
            with torch.cuda.device(self.device):
                for o, n, fo, F in zip(ix.offsets.tolist(), lengths,
                                       fr_off.tolist(), counts.tolist()):
                    if not n:
                        continue
                    place = self.frames_flat[fo * Lc:(fo + F) * Lc]
                    if not composite:
                        place.copy_(raw(self.flat[o:o + n]).reshape(-1))
                        continue
                    # mel + F0: the raw mels (summed one utterance at a time,
                    # as compute_feature_stats sums them), the F0 track, and
                    # the frames assembled in their place
                    a = self.flat[o:o + n][None]
                    mel = raw.mel(a)
                    if mel_stats is not None:
                        mel_stats.update(mel)
                    raw.assemble(mel, (raw.path or raw.tracker)(a).f0,
                                 out=place.view(1, F, Lc))
        elif frames is not None:
            self.frames_flat = filled(list(frames),
                                      [f.shape[0] * Lc for f in frames])
        if norm_kw and norm_kw['normalize'] is not None:
            self._normalize_resident(stats=mel_stats, **norm_kw)
        self._perm_dev = None        # device int32 [rows][P]
        self._perm_pin = None        # its pinned staging rows, their events
        self._perm_e0, self._perm_n = 0, 0   # epochs resident: e0 .. e0 + n - 1
        self._bufs = {}              # output kind -> RING flat device buffers
        self._calls = 0              # batch calls so far: call k uses set k % RING

    def _normalize_resident(self, normalize, clip, allreduce, world,
                            stats=None):
        """Statistics of the resident raw frames (one launch; all shards'
        through `allreduce`), the normaliser, and the frames normalised in
        place, once.  With a mel + F0 front end `stats` holds the sums of the
        raw mel channels already (an n_mels-channel FeatureStats), and the
        mel channels of the resident frames are normalised in place by one
        wn_lc_frames launch; the pitch channels stay as they are."""
        import torch
        from . import features
        composite = self.spec is not None and \
            not isinstance(self.spec, features.MelSpec)
        view = self.frames_flat.view(1, -1, self.Lc)
        with torch.cuda.device(self.device):
            if _wants_stats(normalize, clip, allreduce, world):
                if not composite:
                    stats = features.FeatureStats(self.Lc).update(view)
                if world > 1:
                    stats = features.FeatureStats.from_vector(
                        allreduce(stats.vector()))
                self.feature_stats = stats
            norm = features.Normalizer.from_stats(stats, clip) \
                if normalize == 'corpus' else normalize
            if composite:
                from . import frontend
                frontend.normalize_resident(view[0], self.spec.n_mels, norm)
            else:
                norm(view, out=view)
        self.normalizer = norm
        if self.spec is not None:
            self.spec = self.spec.with_normalizer(norm)

    def compute_feature_stats(self, spec, stats_allreduce=None):
        """features.FeatureStats of the raw (un-normalised) log-mel frames of
        every utterance, for a corpus that keeps no frames: each utterance's
        frames are computed, added to the sums and dropped -- a one-off pass
        with a device peak of one utterance's frames.  With world > 1 the
        sums go through `stats_allreduce` (the sum over ranks of a float64
        vector)."""
        import torch
        from . import features
        if not features.is_spec(spec):
            raise ValueError('compute_feature_stats: spec must be a '
                             'features.MelSpec or a frontend.MelPitchSpec')
        if self.world > 1 and not callable(stats_allreduce):
            raise ValueError('compute_feature_stats: world = %d needs '
                             'stats_allreduce: the statistics of a shard '
                             'differ between ranks' % self.world)
        # (of a mel + F0 front end: its mel part's; an n_mels-channel
        # FeatureStats either way)
        raw = spec.with_normalizer(None) \
            if isinstance(spec, features.MelSpec) else spec.mel
        stats = features.FeatureStats(spec.n_mels)
        with torch.cuda.device(self.device):
            for o, n in zip(self.index.offsets.tolist(),
                            self.index.lengths.tolist()):
                if n:
                    stats.update(raw(self.flat[o:o + n]))
        if self.world > 1:
            stats = features.FeatureStats.from_vector(
                stats_allreduce(stats.vector()))
        return stats

    @property
    def items(self):
        return self.index.items

    def epoch_of(self, step, B):
        return self.index.epoch_of(step, B)

    def plan(self, step, B, T=None):
        return self.index.plan(step, B, T)

    def _perms(self, step, B):
        """(e0, nE, device int32 [nE][P]): the permutations of the epochs
        e0 .. e0 + nE - 1 batch `step` touches.  Those resident from the last
        call move to their rows by device copies; a new one goes up from a
        pinned row, asynchronously."""
        import torch
        e0, nE = self.index.epochs(step, B)
        P = self.index.P
        if self._perm_dev is None or self._perm_dev.shape[0] < nE:
            rows = max(2, nE)
            self._perm_dev = torch.empty((rows, P), dtype=torch.int32,
                                         device=self.device)
            self._perm_pin = [(torch.empty(P, dtype=torch.int32).pin_memory(),
                               torch.cuda.Event()) for _ in range(rows)]
            self._perm_n = 0
        old0, oldn = self._perm_e0, self._perm_n
        if not (old0 <= e0 and e0 + nE <= old0 + oldn):
            for k in range(nE):
                j = e0 + k - old0        # (rows move down: k <= j, ascending)
                if 0 <= k <= j < oldn:
                    if j != k:
                        self._perm_dev[k].copy_(self._perm_dev[j])
                    continue
                host, done = self._perm_pin[k]
                done.synchronize()       # (this row's last upload, long past)
                host.copy_(torch.from_numpy(self.index.perm(e0 + k)))
                self._perm_dev[k].copy_(host, non_blocking=True)
                done.record()
            self._perm_e0, self._perm_n = e0, nE
        return e0, nE, self._perm_dev[e0 - self._perm_e0:]

    def _buffer(self, kind, slot, shape):
        """A view of set `slot`'s buffer for this output, grown to fit."""
        import torch
        n = int(np.prod(shape))
        ring = self._bufs.setdefault(kind, [None] * self.RING)
        if ring[slot] is None or ring[slot].numel() < n:
            ring[slot] = torch.empty(n, dtype=torch.float32,
                                     device=self.device)
        return ring[slot][:n].view(shape)

    def buffer_bytes(self):
        """Device bytes the output buffers hold now."""
        return sum(4 * t.numel() for ring in self._bufs.values()
                   for t in ring if t is not None)

    def plan_args(self, step, B):
        e0, nE, perm = self._perms(step, B)
        ix = self.index
        return (_lib.ptr(self._utt_off), _lib.ptr(self._utt_len),
                int(ix.lengths.shape[0]), _lib.ptr(self._item_utt),
                _lib.ptr(self._item_start), ix.P, _lib.ptr(perm), e0, nE,
                int(step) * int(B), ix.sample_size or 0,
                int(ix.crop == 'random'), ix.seed)

    def gather(self, step, B, out, _args=None, _slot=0):
        """The audio gather of batch `step` alone, into `out` (device
        float32 [B, T], contiguous): one launch on the current stream (with
        history a second, tiny one: the slots' history and lengths as device
        int32 [B] each, left in `device_plan`)."""
        args = _args or self.plan_args(step, B)
        if not self.index.history:
            _lib.call('wn_corpus_gather', _lib.ptr(self.flat),
                      self.flat.numel(), *args, _lib.ptr(out), B,
                      int(out.shape[1]), _lib.stream())
            return
        import torch
        ring = self._bufs.setdefault('plan', [None] * self.RING)
        if ring[_slot] is None or ring[_slot].numel() < 2 * B:
            ring[_slot] = torch.empty(2 * B, dtype=torch.int32,
                                      device=self.device)
        hist, lens = ring[_slot][:B], ring[_slot][B:2 * B]
        _lib.call('wn_corpus_gather_hist', _lib.ptr(self.flat),
                  self.flat.numel(), *args, self.index.history, _lib.ptr(out),
                  _lib.ptr(hist), _lib.ptr(lens), B, int(out.shape[1]),
                  _lib.stream())
        self.device_plan = (hist, lens)

    def batch(self, step, B, T=None, lc='auto'):
        """Batch `step` (module docstring): Batch(audio device float32 [B, T],
        lengths host int64 [B], gc host int32 [B] or None, frames device
        float32 [B, Fw, Lc] + offsets host int64 [B] or rows device float32
        [B, T, Lc], else None; history host int64 [B]: the leading samples of
        every slot that are its history, all 0 without).  T: cut to this many samples (default: the
        longest item's).  lc: 'frames', 'rows', None, or 'auto' = 'frames'
        where the corpus holds frames."""
        import torch
        p = self.index.plan(step, B, T)
        if lc == 'auto':
            lc = 'frames' if self.frames_flat is not None else None
        if lc not in (None, 'frames', 'rows'):
            raise ValueError("batch: lc must be 'frames', 'rows' or None")
        if lc is not None and self.frames_flat is None:
            raise ValueError('batch: the corpus holds no frames (built '
                             'without spec / frames)')
        slot = self._calls % self.RING
        self._calls += 1
        with torch.cuda.device(self.device):
            args = self.plan_args(step, B)
            audio = self._buffer('audio', slot, (B, p.T))
            self.gather(step, B, audio, args, slot)
            frames = offsets = rows = None
            if lc is not None:
                m = LC_CONTEXT_MAX
                Fw = window_frames(p.T, self.hop, m)
                if lc == 'frames':
                    frames = self._buffer('frames', slot, (B, Fw, self.Lc))
                    offsets = self.index.frame_window(
                        p, self.hop, self.frame_counts, m)[2]
                else:
                    rows = self._buffer('rows', slot, (B, p.T, self.Lc))
                H = self.index.history
                _lib.call('wn_corpus_gather_frames_hist' if H else
                          'wn_corpus_gather_frames',
                          _lib.ptr(self.frames_flat),
                          self.frames_flat.numel(), _lib.ptr(self._fr_off),
                          _lib.ptr(self._fr_len), *args, *([H] if H else []),
                          self.hop, m, self.Lc, _lib.ptr(frames), Fw,
                          _lib.ptr(rows), B, p.T, _lib.stream())
        return Batch(audio, p.n.copy(), p.gc, frames, offsets, rows,
                     p.history.copy())


def _wants_stats(normalize, clip, allreduce, world):
    """Whether _normalize_resident sums the resident frames."""
    return normalize == 'corpus' or world == 1 or allreduce is not None


def _check_normalize(normalize, clip, allreduce, world, channels, has_frames):
    """The normalisation keywords, checked before any loading: a dict for
    _setup."""
    from . import features
    if normalize is not None and normalize != 'corpus' and \
            not isinstance(normalize, features.Normalizer):
        raise ValueError("normalize must be None, 'corpus' or a "
                         'features.Normalizer, got %r' % (normalize,))
    if normalize is not None and not has_frames:
        raise ValueError('normalize needs spec (or frames): the corpus holds '
                         'no frames to normalise')
    if clip is not None:
        if normalize != 'corpus':
            raise ValueError("normalize_clip needs normalize='corpus'")
        if isinstance(clip, (bool, np.bool_)) or \
                not isinstance(clip, (int, float, np.integer, np.floating)) \
                or not np.isfinite(clip) or not clip > 0:
            raise ValueError('normalize_clip must be positive, got %r'
                             % (clip,))
    if allreduce is not None and not callable(allreduce):
        raise ValueError('stats_allreduce must be callable or None')
    if normalize == 'corpus' and world > 1 and allreduce is None:
        raise ValueError("normalize='corpus' with world = %d needs "
                         'stats_allreduce: per-shard statistics would '
                         'silently differ between ranks' % world)
    if isinstance(normalize, features.Normalizer) and \
            normalize.n_channels != channels:
        raise ValueError('the normaliser has %d channels, the frames %r'
                         % (normalize.n_channels, channels))
    return dict(normalize=normalize, clip=clip, allreduce=allreduce,
                world=int(world))


def _check_args(sample_size, crop, seed, max_bytes, history=0):
    """CorpusIndex's checks of these, and max_bytes (before any loading)."""
    CorpusIndex([1], None, sample_size, crop, seed, history)
    if not _is_int(max_bytes) or max_bytes < 1:
        raise ValueError('max_bytes must be a positive int, got %r'
                         % (max_bytes,))


def corpus_bytes(samples, frame_floats=0):
    """Device bytes of a corpus: its float32 samples and frame values."""
    return 4 * (int(samples) + int(frame_floats))


def _check_bytes(samples, frame_floats, max_bytes,
                 what='%d bytes on the device'):
    need = corpus_bytes(samples, frame_floats)
    if need > max_bytes:
        raise MemoryError(('the corpus needs ' + what + ', more than '
                           'max_bytes = %d') % (need, max_bytes))
