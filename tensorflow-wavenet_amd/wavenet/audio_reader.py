"""Background audio reader: counterpart of the reference's
wavenet/audio_reader.py (find *.wav recursively, load + resample to mono
float32, RMS silence trim, cut into `sample_size` pieces, speaker id from
`p<id>_<rec>.wav`), feeding the MI355X training loop instead of a
tf.PaddingFIFOQueue.

Same constructor arguments and method names as the reference
(`AudioReader(audio_dir, coord, sample_rate, gc_enabled, sample_size,
silence_threshold, queue_size)`, `dequeue`, `dequeue_gc`, `start_threads`,
`gc_category_cardinality`); new keyword arguments `rank` / `world` shard the
file list per data-parallel rank, `seed` makes the shuffle reproducible.

Local conditioning (`lc_channels`, `lc_hop`): next to every `<clip>.wav` a
`<clip>.npy` of frame-rate features [frames, lc_channels].  They are upsampled
to audio rate by repetition (frame f covers samples f * lc_hop .. + lc_hop - 1),
then silence trimming and piece cutting take the SAME sample indices of audio
and features, so that feature row t of a piece sits beside its sample t.
`dequeue` followed by `dequeue_lc` returns the features of the pieces just
dequeued.

Frames mode (`lc_frames=True`, for a model that upsamples on the device with
its learned network): a piece comes with the frames of its whole clip (the
last frame repeated up to the clip's length, as upsample_lc does) and its
offset, the clip-relative index of its first sample (silence trimming's
start plus k * sample_size; pieces never span files).
`dequeue_lc_frames` returns them for the pieces just dequeued.

librosa is not available in this image: wav I/O is scipy.io.wavfile,
resampling is scipy.signal.resample_poly (librosa's default is a Kaiser-windowed
sinc; the two differ at the 1e-3 level, which only matters if one wants
sample-identical pieces), framing of the RMS energy follows librosa's defaults
(frame 2048, hop 512, centred with reflect padding).
"""
import fnmatch
import os
import queue
import random
import re
import threading
from fractions import Fraction

import numpy as np

_ID_RE = re.compile(r'p([0-9]+)_([0-9]+)\.wav')


class Coordinator(object):
    """Minimal stand-in for tf.train.Coordinator (should_stop/request_stop)."""

    def __init__(self):
        self._stop = threading.Event()

    def should_stop(self):
        return self._stop.is_set()

    def request_stop(self):
        self._stop.set()

    def join(self, threads=(), timeout=5.0):
        for t in threads:
            t.join(timeout)


def find_files(directory, pattern='*.wav'):
    '''Recursively finds all files matching the pattern (sorted).'''
    found = []
    for root, _, names in os.walk(directory):
        for name in fnmatch.filter(names, pattern):
            found.append(os.path.join(root, name))
    return sorted(found)


def category_id_of(filename):
    """Speaker id of a VCTK-style file name `p<id>_<rec>.wav`, else None."""
    m = _ID_RE.findall(os.path.basename(filename))
    return int(m[0][0]) if m else None


def get_category_cardinality(files):
    """(min id, max id) over the files that carry an id."""
    ids = [category_id_of(f) for f in files]
    ids = [i for i in ids if i is not None]
    if not ids:
        return None, None
    return min(ids), max(ids)


def not_all_have_id(files):
    return any(category_id_of(f) is None for f in files)


def load_wav(filename, sample_rate):
    """Mono float32 waveform in [-1, 1] at `sample_rate`."""
    from scipy.io import wavfile
    from scipy.signal import resample_poly
    sr, data = wavfile.read(filename)
    if data.dtype == np.int16:
        audio = data.astype(np.float32) / 32768.0
    elif data.dtype == np.int32:
        audio = data.astype(np.float32) / 2147483648.0
    elif data.dtype == np.uint8:
        audio = (data.astype(np.float32) - 128.0) / 128.0
    else:
        audio = data.astype(np.float32)
    if audio.ndim > 1:
        audio = audio.mean(axis=1)
    if sr != sample_rate:
        frac = Fraction(int(sample_rate), int(sr)).limit_denominator(1000)
        audio = resample_poly(audio, frac.numerator, frac.denominator)
    return np.ascontiguousarray(audio, dtype=np.float32)


def rms_energy(audio, frame_length=2048, hop_length=512):
    """Frame-wise RMS, centred frames with reflect padding."""
    audio = np.asarray(audio, dtype=np.float32)
    if audio.size == 0:
        return np.zeros(0, np.float32)
    pad = frame_length // 2
    mode = 'reflect' if audio.size > pad else 'edge'
    y = np.pad(audio, pad, mode=mode)
    n = 1 + (y.size - frame_length) // hop_length
    idx = np.arange(frame_length)[None, :] + hop_length * np.arange(n)[:, None]
    return np.sqrt(np.mean(y[idx] ** 2, axis=1))


def trim_bounds(audio, threshold, frame_length=2048, hop_length=512):
    '''[lo, hi) of `audio` that trim_silence keeps.'''
    energy = rms_energy(audio, frame_length, hop_length)
    frames = np.nonzero(energy > threshold)[0]
    if frames.size == 0:
        return 0, 0
    return frames[0] * hop_length, frames[-1] * hop_length


def trim_silence(audio, threshold, frame_length=2048, hop_length=512):
    '''Removes silence at the beginning and end of a sample.'''
    lo, hi = trim_bounds(audio, threshold, frame_length, hop_length)
    return audio[lo:hi]


def trim_silence_lc(audio, lc, threshold, frame_length=2048, hop_length=512):
    '''trim_silence of the audio; the audio-rate features [T, Lc] lose the
    same rows.'''
    lo, hi = trim_bounds(audio, threshold, frame_length, hop_length)
    return audio[lo:hi], lc[lo:hi]


def lc_path_of(filename):
    '''The features of `<clip>.wav` live in `<clip>.npy`.'''
    return os.path.splitext(filename)[0] + '.npy'


def upsample_lc(feats, hop, num_samples, lc_channels=None):
    '''Frame-rate features [frames, Lc] -> audio rate [num_samples, Lc] by
    repetition: frame f covers samples f * hop .. f * hop + hop - 1.  The
    audio may run past the last frame by less than one hop (the last frame is
    repeated); anything else is a ValueError.'''
    feats = np.asarray(feats, dtype=np.float32)
    if feats.ndim != 2:
        raise ValueError('local conditioning features must be [frames, '
                         'channels], got shape %s' % (feats.shape,))
    if lc_channels is not None and feats.shape[1] != lc_channels:
        raise ValueError('features have %d channels, expected %d'
                         % (feats.shape[1], lc_channels))
    hop = int(hop)
    if hop <= 0:
        raise ValueError('lc_hop must be positive')
    frames_needed = (int(num_samples) + hop - 1) // hop
    if feats.shape[0] < frames_needed - 1 or feats.shape[0] == 0:
        raise ValueError('%d feature frames at hop %d do not cover %d samples'
                         % (feats.shape[0], hop, num_samples))
    up = np.repeat(feats, hop, axis=0)
    if up.shape[0] < num_samples:
        up = np.concatenate([up, np.repeat(up[-1:], num_samples - up.shape[0],
                                           axis=0)])
    return np.ascontiguousarray(up[:num_samples])


def pad_lc_frames(feats, hop, num_samples, lc_channels=None):
    '''The frames [frames, Lc] that upsample_lc repeats over `num_samples`
    (the last one repeated while the audio runs past it): upsample_lc of the
    result at any length up to num_samples is upsample_lc of `feats`.'''
    feats = np.asarray(feats, dtype=np.float32)
    # (upsample_lc's checks, on a few samples of the same frames)
    upsample_lc(feats, hop, 1, lc_channels)
    hop = int(hop)
    need = (int(num_samples) + hop - 1) // hop
    if feats.shape[0] < need - 1:
        raise ValueError('%d feature frames at hop %d do not cover %d samples'
                         % (feats.shape[0], hop, num_samples))
    if feats.shape[0] < need:
        feats = np.concatenate([feats, np.repeat(
            feats[-1:], need - feats.shape[0], axis=0)])
    return np.ascontiguousarray(feats)


def load_lc(path, hop, num_samples, lc_channels=None):
    '''upsample_lc of the features stored in `path` (.npy).'''
    return upsample_lc(np.load(path), hop, num_samples, lc_channels)


def load_generic_audio(files, sample_rate, rng):
    '''Yields (audio [T,1], filename, category_id) in a shuffled order.'''
    order = list(files)
    rng.shuffle(order)
    for filename in order:
        audio = load_wav(filename, sample_rate)
        yield audio.reshape(-1, 1), filename, category_id_of(filename)


class AudioReader(object):
    '''Generic background audio reader that preprocesses audio files and
    queues fixed-size pieces for the training loop.'''

    def __init__(self,
                 audio_dir,
                 coord,
                 sample_rate,
                 gc_enabled,
                 sample_size=None,
                 silence_threshold=None,
                 queue_size=32,
                 rank=0,
                 world=1,
                 seed=None,
                 *,
                 lc_channels=None,
                 lc_hop=None,
                 lc_frames=False):
        self.audio_dir = audio_dir
        self.sample_rate = sample_rate
        self.coord = coord if coord is not None else Coordinator()
        self.sample_size = sample_size
        self.silence_threshold = silence_threshold
        self.gc_enabled = gc_enabled
        self.lc_channels = lc_channels
        self.lc_hop = lc_hop
        self.lc_enabled = lc_channels is not None
        # frames mode: pieces carry (clip frames, offset), not audio-rate rows
        self.lc_frames = bool(lc_frames) and self.lc_enabled
        if self.lc_enabled and not lc_hop:
            raise ValueError('local conditioning needs lc_hop (samples per '
                             'feature frame)')
        self._last_lc = None
        self._last_lengths = None
        self.threads = []
        self.queue = queue.Queue(maxsize=queue_size)
        self.gc_queue = queue.Queue(maxsize=queue_size) if gc_enabled else None
        self._rng = random.Random(seed)

        files = find_files(audio_dir)
        if not files:
            raise ValueError("No audio files found in '{}'.".format(audio_dir))
        if self.gc_enabled and not_all_have_id(files):
            raise ValueError("Global conditioning is enabled, but file names "
                             "do not conform to pattern having id.")
        if self.gc_enabled:
            # zero-indexed embedding table: largest id + 1 categories
            _, max_id = get_category_cardinality(files)
            self.gc_category_cardinality = max_id + 1
            print("Detected --gc_cardinality={}".format(
                self.gc_category_cardinality))
        else:
            self.gc_category_cardinality = None
        # data-parallel sharding of the file list (new; the reference is
        # single-process)
        self.files = files[rank::world] if world > 1 else files
        if not self.files:
            raise ValueError('rank %d of %d has no audio files' % (rank, world))
        if self.lc_enabled:
            missing = [f for f in self.files if not os.path.exists(lc_path_of(f))]
            if missing:
                raise ValueError('local conditioning is enabled, but %d wav '
                                 'file(s) have no features next to them, e.g. %s'
                                 % (len(missing), lc_path_of(missing[0])))

    # ------------------------------------------------------------- consumer
    def _get(self, q):
        while True:
            try:
                return q.get(timeout=0.2)
            except queue.Empty:
                if self.coord.should_stop() and q.empty():
                    raise RuntimeError('AudioReader stopped')
                if self.threads and not any(t.is_alive() for t in self.threads):
                    raise RuntimeError('AudioReader thread died')

    def dequeue(self, num_elements):
        """float32 tensor [num_elements, T_max, 1], shorter pieces zero-padded
        at the end (tf.PaddingFIFOQueue.dequeue_many semantics)."""
        import torch
        pieces = [self._get(self.queue) for _ in range(num_elements)]
        self._last_lengths = [(p[0] if self.lc_enabled else p).shape[0]
                              for p in pieces]
        if self.lc_enabled:
            # (items are (audio piece, feature piece) pairs: dequeue_lc
            # returns the features of exactly these pieces)
            feats = [f for _, f in pieces]
            pieces = [p for p, _ in pieces]
            if self.lc_frames:
                # [n, F_max, Lc] zero-padded frames + int64 offsets [n]
                fmax = max(f.shape[0] for f, _ in feats)
                fr = np.zeros((num_elements, fmax, self.lc_channels),
                              np.float32)
                for i, (f, _) in enumerate(feats):
                    fr[i, :f.shape[0]] = f
                self._last_lc = (torch.from_numpy(fr), torch.tensor(
                    [o for _, o in feats], dtype=torch.int64))
            else:
                tmax = max(p.shape[0] for p in pieces)
                lc = np.zeros((num_elements, tmax, self.lc_channels),
                              np.float32)
                for i, f in enumerate(feats):
                    lc[i, :f.shape[0]] = f
                self._last_lc = torch.from_numpy(lc)
        tmax = max(p.shape[0] for p in pieces)
        out = np.zeros((num_elements, tmax, 1), np.float32)
        for i, p in enumerate(pieces):
            out[i, :p.shape[0], :] = p
        return torch.from_numpy(out)

    def dequeue_lengths(self, num_elements):
        """int64 [num_elements]: the unpadded sample counts of the pieces the
        last `dequeue(num_elements)` returned (WaveNetModel.loss's `lengths`;
        everything behind them in dequeue's rows, and in the features' or
        frames', is zero padding)."""
        import torch
        n = self._last_lengths
        if n is None or len(n) != num_elements:
            raise ValueError('dequeue_lengths(%d) must follow dequeue(%d)'
                             % (num_elements, num_elements))
        self._last_lengths = None
        return torch.tensor(n, dtype=torch.int64)

    def dequeue_lc(self, num_elements):
        """float32 [num_elements, T_max, lc_channels]: the audio-rate features
        of the pieces the last `dequeue(num_elements)` returned (zero-padded
        like them); row t sits beside sample t."""
        if not self.lc_enabled or self.lc_frames:
            raise ValueError('AudioReader was built without lc_channels'
                             if not self.lc_enabled else
                             'frames mode: use dequeue_lc_frames')
        return self._take_lc(num_elements)

    def dequeue_lc_frames(self, num_elements):
        """Frames mode: (frames float32 [num_elements, F_max, lc_channels],
        offsets int64 [num_elements]) of the pieces the last
        `dequeue(num_elements)` returned: sample t of piece i sits at position
        offsets[i] + t of its clip, whose frame is (offsets[i] + t) // lc_hop
        (frames zero-padded behind each clip's own)."""
        if not self.lc_frames:
            raise ValueError('AudioReader was built without lc_frames')
        return self._take_lc(num_elements)

    def _take_lc(self, num_elements):
        lc = self._last_lc
        n = None if lc is None else \
            (lc[1].shape[0] if isinstance(lc, tuple) else lc.shape[0])
        if n != num_elements:
            raise ValueError('dequeue_lc(%d) must follow dequeue(%d)'
                             % (num_elements, num_elements))
        self._last_lc = None
        return lc

    def dequeue_gc(self, num_elements):
        import torch
        ids = [self._get(self.gc_queue) for _ in range(num_elements)]
        return torch.tensor(ids, dtype=torch.int32)

    # ------------------------------------------------------------- producer
    def _put(self, q, item):
        while not self.coord.should_stop():
            try:
                q.put(item, timeout=0.2)
                return True
            except queue.Full:
                continue
        return False

    def iter_pieces(self):
        """One pass over the (shuffled) files: (piece [n, 1], category id,
        feature piece [n, lc_channels] or None) in queue order."""
        buffer_ = np.zeros((0,), np.float32)
        lc_buf = np.zeros((0, self.lc_channels or 0), np.float32)
        for audio, filename, category_id in load_generic_audio(
                self.files, self.sample_rate, self._rng):
            lc = None
            if self.lc_frames:
                yield from self._frame_pieces(audio[:, 0], filename,
                                              category_id)
                continue
            if self.lc_enabled:
                lc = load_lc(lc_path_of(filename), self.lc_hop, audio.shape[0],
                             self.lc_channels)
            if self.silence_threshold is not None:
                if lc is not None:
                    a, lc = trim_silence_lc(audio[:, 0], lc,
                                            self.silence_threshold)
                else:
                    a = trim_silence(audio[:, 0], self.silence_threshold)
                audio = a.reshape(-1, 1)
                if audio.size == 0:
                    print("Warning: {} was ignored as it contains only "
                          "silence. Consider decreasing trim_silence "
                          "threshold, or adjust volume of the audio."
                          .format(filename))
            if self.sample_size:
                # cut into fixed-size pieces (the last piece of a file is
                # short; consecutive files are concatenated like the
                # reference's running buffer); features at the same indices
                buffer_ = np.append(buffer_, audio)
                if lc is not None:
                    lc_buf = np.concatenate([lc_buf, lc])
                while len(buffer_) > 0:
                    piece = buffer_[:self.sample_size].reshape(-1, 1)
                    lp = lc_buf[:self.sample_size].copy() if lc is not None \
                        else None
                    yield piece.copy(), category_id, lp
                    buffer_ = buffer_[self.sample_size:]
                    if lc is not None:
                        lc_buf = lc_buf[self.sample_size:]
            elif audio.size:
                yield audio, category_id, lc

    def _frame_pieces(self, audio, filename, category_id):
        """iter_pieces of one file in frames mode: (piece [n, 1], category
        id, (clip frames, offset of the piece's first sample))."""
        frames = pad_lc_frames(np.load(lc_path_of(filename)), self.lc_hop,
                               audio.shape[0], self.lc_channels)
        lo = 0
        if self.silence_threshold is not None:
            lo, hi = trim_bounds(audio, self.silence_threshold)
            audio = audio[lo:hi]
            if audio.size == 0:
                print("Warning: {} was ignored as it contains only "
                      "silence. Consider decreasing trim_silence "
                      "threshold, or adjust volume of the audio."
                      .format(filename))
        step = self.sample_size or max(audio.size, 1)
        for k in range(0, audio.size, step):
            yield (audio[k:k + step].reshape(-1, 1).copy(), category_id,
                   (frames, int(lo + k)))

    def thread_main(self, sess=None):
        while not self.coord.should_stop():      # many passes over the data
            for piece, category_id, lc in self.iter_pieces():
                if self.coord.should_stop():
                    return
                item = (piece, lc) if self.lc_enabled else piece
                if not self._put(self.queue, item):
                    return
                if self.gc_enabled and not self._put(self.gc_queue,
                                                     category_id):
                    return

    def start_threads(self, sess=None, n_threads=1):
        for _ in range(n_threads):
            thread = threading.Thread(target=self.thread_main, args=(sess,))
            thread.daemon = True  # Thread will close when parent quits.
            thread.start()
            self.threads.append(thread)
        return self.threads
