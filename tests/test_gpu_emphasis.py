"""Pre-emphasis and de-emphasis on the device (wavenet/emphasis.py,
csrc/wn_features.hip): the pre-emphasis bit for bit against the numpy float32
rule; the de-emphasis scan against the float64 recurrence within the derived
bound of tests/emph_ref.py, at every length around the scan's chunk, alone
and inside a batch, in pieces with the carry, in place; and the training
sources' pre-emphasis step (wavenet/training.py) on a device corpus."""
import numpy as np
import pytest
import torch

import emph_ref as R

pytestmark = pytest.mark.gpu

ALPHAS = (0.5, 0.97, 0.995)


def _bits(t):
    return (t.detach().cpu().numpy() if hasattr(t, 'detach')
            else np.asarray(t)).astype(np.float32).tobytes()


def _signal(rng, n):
    """Uniform noise with two decaying sinusoid bursts."""
    x = rng.uniform(-1, 1, n)
    for k in range(2):
        s = int(rng.integers(0, max(1, n - 1)))
        t = np.arange(n - s)
        x[s:] += 2.0 * np.exp(-t / 300.0) * np.sin(0.05 * (k + 1) * t)
    return x.astype(np.float32)


def _within(got, e, alpha, lengths=None, initial=None, factor=1.0):
    """got (device or numpy [B, T] or [T]) against the float64 recurrence."""
    y, bound = R.de64(e, alpha, lengths, initial)
    err = np.abs(got.detach().cpu().numpy().astype(np.float64) - y)
    worst = float((err / bound.clip(min=2.0 ** -126)).max())
    print('alpha %g shape %s: worst error / bound = %.3f'
          % (alpha, np.shape(e), worst))
    assert (err <= factor * bound).all(), worst


@pytest.fixture(scope='module')
def emph(hip_lib):
    from wavenet.emphasis import Emphasis
    return Emphasis


@pytest.fixture(scope='module')
def C(emph):
    c = emph.chunk()
    assert c >= 64 and c % 64 == 0
    return c


@pytest.fixture(scope='module')
def clips(emph, C):
    """Clips of C - 1, C, C + 1, 2 C + 1 and 5 C + 3 samples at alpha 0.97:
    (lengths, inputs [5, 5 C + 3] zero padded, each clip's output alone)."""
    rng = np.random.default_rng(11)
    n = np.array([C - 1, C, C + 1, 2 * C + 1, 5 * C + 3])
    e = np.zeros((5, int(n.max())), np.float32)
    for j in range(5):
        e[j, :n[j]] = _signal(rng, int(n[j]))
    f = emph(0.97)
    alone = [f.de(e[j, :n[j]]) for j in range(5)]
    return n, e, alone


# ------------------------------------------------------------ pre-emphasis
@pytest.mark.parametrize('alpha', ALPHAS)
def test_pre_is_the_numpy_float32_rule(emph, alpha):
    rng = np.random.default_rng(1)
    B, T = 5, 1031
    x = rng.uniform(-1, 1, (B, T)).astype(np.float32)
    n = np.array([T, 1, 2, 517, 1030])
    f = emph(alpha)
    assert _bits(f.pre(x)) == _bits(f.reference_pre(x))
    assert _bits(f.pre(x, n)) == _bits(f.reference_pre(x, n))
    assert _bits(f.pre(x[3])) == _bits(f.reference_pre(x[3]))
    if alpha == 0.5:
        return                    # (alpha * x is exact: nothing to fuse)
    # not an FMA: the fused value differs somewhere in 5155 samples
    prev = np.concatenate([np.zeros((B, 1)), x[:, :-1].astype(np.float64)], 1)
    fused = (x.astype(np.float64) - float(f.alpha32) * prev
             ).astype(np.float32)
    assert fused.tobytes() != f.reference_pre(x).tobytes()


def test_pre_leading_dimensions_nan_padding_and_identity(emph):
    rng = np.random.default_rng(2)
    B, T = 4, 300
    n = np.array([300, 7, 150, 299])
    x = rng.uniform(-1, 1, (B, T)).astype(np.float32)
    f = emph(0.97)
    want = f.reference_pre(x, n)
    dirty = x.copy()
    for b in range(B):
        dirty[b, n[b]:] = np.nan
    big = torch.full((B, T + 37), float('nan'), device='cuda')
    big[:, :T] = torch.from_numpy(dirty).cuda()
    out_big = torch.full((B, T + 5), 7.0, device='cuda')
    got = f.pre(big[:, :T], n, out=out_big[:, :T])
    assert got.data_ptr() == out_big.data_ptr()
    assert _bits(got) == _bits(want)
    assert not np.isnan(got.cpu().numpy()).any()
    assert (out_big[:, T:] == 7.0).all()          # nothing behind T is touched
    for b in range(B):
        assert not got[b, n[b]:].any()
    z = emph(0.0)
    assert _bits(z.pre(x)) == x.tobytes()
    assert _bits(z.de(x)) == x.tobytes()
    with pytest.raises(ValueError):
        f.pre(big[:, :T], out=big[:, 1:T + 1])    # overlapping


# ------------------------------------------------------------- de-emphasis
@pytest.mark.parametrize('alpha', ALPHAS)
def test_de_ragged_batch_of_every_length(emph, alpha):
    rng = np.random.default_rng(3)
    B = T = 130
    n = np.arange(1, B + 1)
    e = rng.uniform(-1, 1, (B, T)).astype(np.float32)
    dirty = e.copy()
    for b in range(B):
        dirty[b, n[b]:] = np.nan
    f = emph(alpha)
    got, last = f.de(dirty, n, return_last=True)
    g = got.cpu().numpy()
    assert not np.isnan(g).any()
    for b in range(B):
        assert not g[b, n[b]:].any()
    _within(got, np.where(np.arange(T)[None] < n[:, None], e, 0), alpha, n)
    assert _bits(last) == g[np.arange(B), n - 1].tobytes()


def test_de_clips_around_the_chunk(emph, clips):
    n, e, alone = clips
    got = np.zeros_like(e)
    for j in range(5):
        got[j, :n[j]] = alone[j].cpu().numpy()
    _within(torch.from_numpy(got), e, 0.97, n)


def test_de_clip_bits_do_not_depend_on_the_batch(emph, clips):
    n, e, alone = clips
    f = emph(0.97)
    rng = np.random.default_rng(4)
    for j in range(5):
        T = int(n[j]) + 13
        batch = torch.full((4, T + 3), float('nan'), device='cuda')
        lengths = np.array([5, T, int(n[j]), max(1, int(n[j]) // 2)])
        batch[:, :T] = torch.from_numpy(
            rng.uniform(-1, 1, (4, T)).astype(np.float32)).cuda()
        batch[2, :n[j]] = torch.from_numpy(e[j, :n[j]]).cuda()
        got = f.de(batch[:, :T], lengths)          # (ld = T + 3)
        assert _bits(got[2, :n[j]]) == _bits(alone[j]), int(n[j])
        assert not got[2, n[j]:].any()


@pytest.mark.parametrize('alpha', ALPHAS)
def test_de_impulse_and_constant_across_three_chunks(emph, C, alpha):
    T = 3 * C
    e = np.zeros((2, T), np.float32)
    e[0, 0] = 1.0
    e[1] = 1.0
    f = emph(alpha)
    got = f.de(e)
    _within(got, e, alpha)
    a = R.alpha64(alpha)
    # the constant approaches 1 / (1 - a), from which y[T - 1] is a^T / (1 - a)
    # away; the impulse decays and stays >= 0
    assert abs(float(got[1, -1]) - 1.0 / (1.0 - a)) <= \
        R.de64(e[1], alpha)[1][-1] + a ** T / (1.0 - a)
    assert float(got[0, -1]) >= 0.0


def test_de_in_pieces_with_the_carry(emph, C, clips):
    n, e, alone = clips
    f = emph(0.97)
    x = e[4]
    whole = alone[4]
    for piece, exact in ((C + 7, False), (C, True), (2 * C, True)):
        parts, last = [], None
        for s in range(0, x.shape[0], piece):
            y, last = f.de(x[s:s + piece], initial=last, return_last=True)
            parts.append(y)
        got = torch.cat(parts)
        assert _bits(last) == _bits(got[-1:])
        if exact:
            assert _bits(got) == _bits(whole), piece
        else:
            _within(got, x, 0.97, factor=2.0)
    # a batch's carries: [B] in, [B] out
    two = np.stack([x[:C + 9], x[5:C + 14]])
    y0, l0 = f.de(two[:, :C], return_last=True)
    y1 = f.de(two[:, C:], initial=l0)
    _within(torch.cat([y0, y1], 1), two, 0.97, factor=2.0)


def test_de_in_place_is_out_of_place(emph, clips):
    n, e, alone = clips
    f = emph(0.97)
    buf = torch.from_numpy(e).cuda()
    want = f.de(buf, n)
    got = f.de(buf, n, out=buf)
    assert got is buf
    assert _bits(got) == _bits(want)
    for j in range(5):
        assert _bits(got[j, :n[j]]) == _bits(alone[j])


def test_de_inverts_pre(emph, C):
    x = _signal(np.random.default_rng(6), C + 77)
    f = emph(0.97)
    back = f.de(f.pre(x))
    # pre's two roundings per sample are one more error term of the filter
    y, bound = R.de64(R.pre64(x, 0.97), 0.97)
    e = f.reference_pre(x).astype(np.float64)
    _, b2 = R.de64(e, 0.97)
    slack = R.de64(2.0 ** -23 * (np.abs(x) + np.abs(e)), 0.97)[0]
    assert (np.abs(back.cpu().numpy() - x) <= b2 + slack).all()


# ------------------------------------------------- the training sources' step
def test_corpus_source_take_pre_emphasises_a_copy(emph, tmp_path):
    from scipy.io import wavfile
    from wavenet import training
    from wavenet.corpus import DeviceCorpus
    from wavenet.features import MelSpec
    rng = np.random.default_rng(8)
    for i in range(4):
        m = 700 + 211 * i
        x = 0.6 * np.sin(2 * np.pi * 220.0 * (i + 1) * np.arange(m) / 16000.0) \
            + 0.05 * rng.standard_normal(m)
        wavfile.write(str(tmp_path / ('c%d.wav' % i)), 16000,
                      (np.clip(x, -1, 1) * 32767).astype(np.int16))
    spec = MelSpec(16000, n_fft=64, hop=16, n_mels=8)
    corpus = DeviceCorpus(str(tmp_path), 16000, False, sample_size=500,
                          silence_threshold=None, spec=spec)
    f = emph(0.97)
    B = 3
    src = training.CorpusSource(corpus, {}, lengths=True, lc='frames',
                                emphasis=f)
    T, lengths, _ = src.plan(0, B)
    raw = corpus.batch(0, B)
    raw_audio, raw_frames = raw.audio.clone(), raw.frames.clone()
    a0, fr0, off0 = src.take(0, B, T)
    assert _bits(a0) == f.reference_pre(raw_audio.cpu().numpy(),
                                        raw.lengths).tobytes()
    assert _bits(fr0) == _bits(raw_frames)
    assert np.array_equal(off0, raw.offsets)
    # the corpus's own tensors are not rewritten
    again = corpus.batch(0, B)
    assert _bits(again.audio) == _bits(raw_audio)
    a1, _, _ = src.take(1, B, src.plan(1, B)[0])
    lo0, hi0 = a0.data_ptr(), a0.data_ptr() + 4 * a0.numel()
    lo1, hi1 = a1.data_ptr(), a1.data_ptr() + 4 * a1.numel()
    assert hi0 <= lo1 or hi1 <= lo0
    assert _bits(a0) == f.reference_pre(raw_audio.cpu().numpy(),
                                        raw.lengths).tobytes()
    # without an Emphasis the source hands the corpus's batch through
    plain = training.CorpusSource(corpus, {}, lengths=True, lc='frames')
    p0, _, _ = plain.take(0, B, T)
    assert _bits(p0) == _bits(raw_audio)
