"""Feature normalisation on the device (csrc/wn_features.hip through
wavenet/features.py and wavenet/corpus.py): wn_feature_stats against float64
numpy within the bound of two summation orders, wn_feature_normalize bit for
bit against tests/featnorm_ref.py, MelSpec and DeviceCorpus with a normaliser,
and the loss on a corpus's normalised frames."""
import numpy as np
import pytest
import torch

import featnorm_ref as R
import mel_ref

pytestmark = pytest.mark.gpu

NAN = float('nan')
# (B, F, C): one element; row counts around the partial count (256) that are
# no multiple of it, scalar path; the same with 80 channels and three clips;
# the 16-byte path at a small C; the channel cap (128 lanes of 4 channels: one
# trip of the partials kernel's channel loop); the scalar path above 256
# channels (256 lanes of 1 channel: two trips, the second with 45 and with 6
# live lanes)
SHAPES = [(1, 1, 1), (1, 255, 3), (1, 257, 3), (3, 86, 80), (2, 300, 4),
          (1, 40, 512), (1, 40, 301), (2, 300, 262)]
WN_ERR_BAD_SHAPE, WN_ERR_MISALIGNED = -1, -3


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(got, want):
    g, w = _bits(got), _bits(want)
    return g.shape == w.shape and bool((g == w).all())


def _same_but_nans(got, want):
    """Bit for bit; a NaN of any payload where the other holds a NaN."""
    if isinstance(got, torch.Tensor):
        got = got.detach().cpu().numpy()
    gn, wn = np.isnan(got), np.isnan(want)
    return got.shape == want.shape and bool((gn == wn).all()) and \
        bool((_bits(got)[~gn] == _bits(want)[~wn]).all())


_DATA = {}


def _data(shape):
    """float32 [B, F, C] shaped like log-mel frames (mean -10, std 11), computed
    once, shared, never written to."""
    if shape not in _DATA:
        rng = np.random.default_rng(sum(shape))
        x = (rng.standard_normal(shape) * 11 - 10).astype(np.float32)
        x.setflags(write=False)
        _DATA[shape] = x
    return _DATA[shape]


def _ragged(B, F):
    """A clip without frames, one with all of them, one in between."""
    return {1: [F // 2], 2: [0, F], 3: [0, F, F // 3]}[B]


def _poisoned(x, nframes):
    """x with NaN behind every clip's real frames."""
    x = x.copy()
    if nframes is not None:
        x[~R.real_mask(x.shape[0], x.shape[1], nframes)] = NAN
    return x


def _raw_stats(x, nframes, acc):
    """wn_feature_stats itself on a device tensor: acc (device float64
    [2, C]) is accumulated into."""
    from wavenet import _lib
    B, F, C = x.shape
    parts = _lib.load().wn_feature_stats_partials_count()
    scratch = torch.full((parts * 2 * C,), NAN, dtype=torch.float64,
                         device=x.device)
    nd = None if nframes is None else \
        torch.tensor(nframes, dtype=torch.int32, device=x.device)
    _lib.call('wn_feature_stats', _lib.ptr(x), B, F, C, _lib.ptr(nd),
              _lib.ptr(acc), _lib.ptr(scratch), _lib.stream())
    torch.cuda.synchronize()
    return acc.cpu().numpy()


# ------------------------------------------------------------ wn_feature_stats
@pytest.mark.parametrize('ragged', [False, True], ids=['whole', 'ragged'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_stats_match_float64_numpy(hip_lib, shape, ragged):
    from wavenet import features
    B, F, C = shape
    nf = _ragged(B, F) if ragged else None
    x = _poisoned(_data(shape), nf)
    n, s1, s2, a1, a2 = R.sums(_data(shape), nf)
    st = features.FeatureStats(C).update(x, nf)
    cnt, g1, g2 = st.sums()
    assert cnt == n and g1.dtype == np.float64 and g1.shape == (C,)
    e1, e2 = np.abs(g1 - s1), np.abs(g2 - s2)
    print('%s n %d: max |S - ref| %.3g (bound %.3g), squares %.3g (%.3g)'
          % (shape, n, e1.max(), R.sum_bound(n, a1).max(), e2.max(),
             R.sum_bound(n, a2).max()))
    assert np.isfinite(g1).all() and np.isfinite(g2).all()   # (no NaN read)
    assert (e1 <= R.sum_bound(n, a1)).all()
    assert (e2 <= R.sum_bound(n, a2)).all()
    # the same input again: the same bits
    again = features.FeatureStats(C).update(x, nf).sums()
    assert _same_bits(again[1], g1) and _same_bits(again[2], g2)
    # one clip alone, as [F, C]
    if B > 1:
        one = features.FeatureStats(C).update(x[1]).sums()
        w = R.sums(_data(shape)[1:2])
        assert one[0] == F and (np.abs(one[1] - w[1]) <=
                                R.sum_bound(F, w[3])).all()


def test_stats_accumulate_in_order(hip_lib):
    from wavenet import features
    shape = (2, 300, 4)
    x = _data(shape)
    a = features.FeatureStats(4).update(x[:1]).sums()
    b = features.FeatureStats(4).update(x[1:], [123]).sums()
    both = features.FeatureStats(4).update(x[:1]).update(x[1:], [123])
    cnt, s1, s2 = both.sums()
    assert cnt == 300 + 123
    assert _same_bits(s1, a[1] + b[1]) and _same_bits(s2, a[2] + b[2])
    # an accumulator that starts non-zero: acc + the launch's own sum
    dev = torch.tensor(x).cuda()            # (a copy: x is read-only)
    fresh = _raw_stats(dev, None, torch.zeros((2, 4), dtype=torch.float64,
                                              device='cuda'))
    start = np.array([[1e6, -3.5, 0.25, 7.0], [1e9, 2.0, -1.0, 0.5]])
    got = _raw_stats(dev, None, torch.from_numpy(start).cuda())
    assert _same_bits(got, start + fresh)
    # merged with what a host gave
    host = features.FeatureStats.from_sums(5, np.ones(4), np.full(4, 2.0))
    host.update(x[:1])
    assert host.count == 305 and _same_bits(host.sums()[1], 1.0 + a[1])


def test_bad_arguments_return_codes_before_any_launch(hip_lib):
    from wavenet import _lib
    lib = _lib.load()
    buf = torch.zeros(4096, dtype=torch.float32, device='cuda')
    dbl = torch.zeros(256 * 2 * 512 + 2, dtype=torch.float64, device='cuda')
    p, d, s = buf.data_ptr(), dbl.data_ptr(), _lib.stream()
    assert lib.wn_feature_stats_partials_count() == 256
    for B, F, C in ((1, 1, 0), (1, 1, 513), (0, 1, 4), (1, 0, 4), (-1, 4, 4),
                    (65536, 32768, 4)):
        assert lib.wn_feature_stats(p, B, F, C, None, d, d + 8192, s) == \
            WN_ERR_BAD_SHAPE
        assert lib.wn_feature_normalize(p, p, B, F, C, None, p, p, -1.0, 1.0,
                                        s) == WN_ERR_BAD_SHAPE
    assert lib.wn_feature_normalize(p, p, 1, 4, 4, None, p, p, 1.0, -1.0,
                                    s) == WN_ERR_BAD_SHAPE
    for args in ((p + 4, 1, 4, 4, None, d, d + 8192),
                 (p + 2, 1, 4, 3, None, d, d + 8192),
                 (p, 1, 4, 4, p + 2, d, d + 8192),
                 (p, 1, 4, 4, None, d + 4, d + 8192),
                 (p, 1, 4, 4, None, d, d + 8196)):
        assert lib.wn_feature_stats(*args, s) == WN_ERR_MISALIGNED
    for args in ((p + 4, p, 1, 4, 4, None, p, p), (p, p + 8, 1, 4, 4, None, p, p),
                 (p, p, 1, 4, 4, None, p + 4, p), (p, p, 1, 4, 4, None, p, p + 4),
                 (p + 2, p, 1, 4, 3, None, p, p), (p, p, 1, 4, 3, p + 1, p, p)):
        assert lib.wn_feature_normalize(*args, -1.0, 1.0, s) == \
            WN_ERR_MISALIGNED
    # 4-byte alignment is enough where C % 4 != 0
    assert lib.wn_feature_normalize(p + 4, p + 4, 1, 4, 3, None, p + 4, p + 4,
                                    -1.0, 1.0, s) == 0
    torch.cuda.synchronize()
    assert not buf.any() and not dbl.any()


# -------------------------------------------------------- wn_feature_normalize
def _normalizer(C, clamp, seed=0):
    from wavenet import features
    rng = np.random.default_rng(seed)
    shift = (rng.standard_normal(C) * 2 - 10).astype(np.float32)
    scale = (1.0 / rng.uniform(2.0, 12.0, C)).astype(np.float32)
    scale[::3] *= -1                                    # (any sign)
    return features.Normalizer(shift, scale, *((-1.5, 1.0) if clamp else
                                               (None, None)))


@pytest.mark.parametrize('clamp', [True, False], ids=['clamp', 'noclamp'])
@pytest.mark.parametrize('ragged', [False, True], ids=['whole', 'ragged'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_normalize_is_the_restated_rule_bit_for_bit(hip_lib, shape, ragged,
                                                    clamp):
    B, F, C = shape
    nf = _ragged(B, F) if ragged else None
    x = _poisoned(_data(shape), nf)
    x[-1, 0, C // 2] = NAN            # a NaN in a real frame (if it is one)
    x[0, F // 4, 0] = np.inf
    norm = _normalizer(C, clamp)
    lo = -np.inf if norm.lo is None else norm.lo
    hi = np.inf if norm.hi is None else norm.hi
    want = R.normalize(x, norm.shift, norm.scale, lo, hi, nf)
    assert np.array_equal(np.isnan(want), np.isnan(norm.reference(x, nf)))
    if clamp and B * F > 1:
        assert (want == np.float32(lo)).any() and (want == np.float32(hi)).any()
    # out of place, into a buffer full of NaN: every float is written
    dev = torch.from_numpy(x).cuda()
    out = torch.full_like(dev, NAN)
    assert norm(dev, nf, out=out) is out
    torch.cuda.synchronize()
    assert _same_but_nans(out, want)
    real = R.real_mask(B, F, nf)
    assert not _bits(out.cpu().numpy()[~real]).any()     # exact +0
    if real[-1, 0] and np.isnan(x[-1, 0, C // 2]):
        assert bool(torch.isnan(out[-1, 0, C // 2]))
    fresh = norm(dev, nf)
    assert fresh.data_ptr() != dev.data_ptr() and _same_but_nans(fresh, want)
    # from the host, and a single clip [F, C]
    assert _same_but_nans(norm(x, nf), want)
    one = norm(x[0], None if nf is None else nf[:1])
    assert one.shape == (F, C) and _same_but_nans(one, want[0])
    # in place
    assert norm(dev, nf, out=dev) is dev
    torch.cuda.synchronize()
    assert _same_but_nans(dev, want)


@pytest.mark.parametrize('shape', [(1, 255, 3), (1, 257, 3), (1, 1, 1)],
                         ids=str)
def test_normalize_from_a_view_off_by_four_bytes(hip_lib, shape):
    """C % 4 != 0: the scalar path needs 4-byte alignment only."""
    B, F, C = shape
    x = _data(shape)
    norm = _normalizer(C, True, seed=1)
    flat = torch.zeros(x.size + 1, dtype=torch.float32, device='cuda')
    view = flat[1:].view(B, F, C)
    view.copy_(torch.tensor(x))
    assert view.data_ptr() % 16 == 4
    want = R.normalize(x, norm.shift, norm.scale, norm.lo, norm.hi)
    out = torch.full((x.size + 1,), NAN, dtype=torch.float32, device='cuda')
    got = norm(view, out=out[1:].view(B, F, C))
    torch.cuda.synchronize()
    assert _same_bits(got, want) and bool(torch.isnan(out[0]))
    from wavenet import features
    st = features.FeatureStats(C).update(view).sums()
    assert _same_bits(st[1], features.FeatureStats(C).update(x).sums()[1])


# ------------------------------------------------------ MelSpec with a normaliser
MEL = dict(sample_rate=8000, n_fft=64, hop=16, win_length=64, n_mels=8)


def _audio(lengths, seed=3):
    rng = np.random.default_rng(seed)
    T = max(lengths)
    x = rng.uniform(-0.1, 0.1, (len(lengths), T)) + \
        0.4 * np.sin(0.3 * np.arange(T))[None, :]
    return x.astype(np.float32)


def test_melspec_with_a_normalizer(hip_lib):
    from wavenet import features
    lengths = [5, 100, 33]
    audio, hop = _audio(lengths), MEL['hop']
    nf = [-(-n // hop) for n in lengths]
    raw = features.MelSpec(MEL['sample_rate'], n_fft=64, hop=16, n_mels=8)
    fr = raw(audio, lengths)
    norm = features.Normalizer.from_stats(
        features.FeatureStats(8).update(fr, nf), clip=1.5)
    spec = raw.with_normalizer(norm)
    got = spec(audio, lengths)
    torch.cuda.synchronize()
    assert got.shape == (3, 7, 8)
    assert _same_bits(got, norm(fr, nf))
    assert _same_bits(got, R.normalize(fr.cpu().numpy(), norm.shift,
                                       norm.scale, norm.lo, norm.hi, nf))
    assert not _bits(got)[~R.real_mask(3, 7, nf)].any()
    assert _same_bits(raw(audio, lengths), fr)           # (raw is untouched)
    # the float64 oracle, normalised in float64
    ref = mel_ref.logmel_batch(audio, lengths, **MEL)
    want = np.clip((ref - norm.shift.astype(np.float64)) *
                   norm.scale.astype(np.float64), norm.lo, norm.hi)
    want[~R.real_mask(3, 7, nf)] = 0.0
    err = np.abs(got.cpu().numpy() - want).max()
    # (the raw frames' tolerance of tests/test_gpu_features.py, scaled)
    tol = mel_ref.MEL_TOL * np.abs(norm.scale).max()
    print('max error against the normalised oracle %.3g (tolerance %.3g)'
          % (err, tol))
    assert err <= tol
    assert (np.abs(want) == 1.5).any()                   # (the clamp acts)
    # a clip's frames do not depend on the batch it was computed in
    for b, n in enumerate(lengths):
        alone = spec(audio[b, :n])
        assert _same_bits(alone, got[b, :nf[b]])
    # without lengths every frame is real
    assert _same_bits(spec(audio), norm(raw(audio)))


# ------------------------------------------------- DeviceCorpus, normalize='corpus'
UTT = [100, 250, 400, 550, 700]


def _utterances():
    rng = np.random.default_rng(9)
    return [(0.3 * np.sin(0.05 * (k + 2) * np.arange(n)) +
             0.05 * rng.standard_normal(n)).astype(np.float32) *
            np.float32(0.2 + 0.2 * k) for k, n in enumerate(UTT)]


def _mel():
    from wavenet import features
    return features.MelSpec(8000, n_fft=64, hop=16, n_mels=8)


@pytest.fixture(scope='module')
def corpora(hip_lib):
    """(utterances, spec, normalised corpus, its un-normalised twin)."""
    from wavenet.corpus import DeviceCorpus
    utts, spec = _utterances(), _mel()
    kw = dict(sample_size=150, crop='random', seed=7)
    corpus = DeviceCorpus.from_arrays(utts, spec=spec, normalize='corpus',
                                      normalize_clip=3.0, **kw)
    twin = DeviceCorpus.from_arrays(utts, spec=spec, **kw)
    torch.cuda.synchronize()
    return utts, spec, corpus, twin


def test_corpus_statistics_and_resident_frames(corpora):
    from wavenet import features
    from wavenet.corpus import DeviceCorpus
    utts, spec, corpus, twin = corpora
    assert twin.normalizer is None and twin.feature_stats is None
    raw = twin.frames_flat.cpu().numpy().reshape(1, -1, 8)
    n, s1, s2, a1, a2 = R.sums(raw)
    assert n == sum(-(-u // 16) for u in UTT)
    # the statistics of the raw frames, one utterance at a time
    each = features.FeatureStats(8)
    for u in utts:
        each.update(spec(u))
    cnt, g1, g2 = corpus.feature_stats.sums()
    assert cnt == n == each.count
    for got in (corpus.feature_stats, each):
        assert (np.abs(got.sums()[1] - s1) <= R.sum_bound(n, a1)).all()
        assert (np.abs(got.sums()[2] - s2) <= R.sum_bound(n, a2)).all()
    norm = corpus.normalizer
    want = features.Normalizer.from_stats(corpus.feature_stats, clip=3.0)
    assert norm.entry() == want.entry() and (norm.lo, norm.hi) == (-3.0, 3.0)
    shift, scale = R.shift_scale(cnt, g1, g2)
    assert _same_bits(norm.shift, shift) and _same_bits(norm.scale, scale)
    assert corpus.spec.normalizer is norm and spec.normalizer is None
    assert features.checkpoint_entry(corpus.spec)['normalizer'] == norm.entry()
    # the resident frames: normalised once
    assert _same_bits(corpus.frames_flat,
                      norm.reference(raw).reshape(-1))
    assert _same_bits(corpus.frames_flat, R.normalize(
        raw, norm.shift, norm.scale, -3.0, 3.0).reshape(-1))
    flat = corpus.frames_flat.cpu().numpy().reshape(-1, 8)
    assert np.abs(flat.mean(0)).max() < 0.25 and \
        0.5 < flat.std(0).min() and flat.std(0).max() < 1.1
    # a corpus that keeps no frames: the same sums from a pass of its own
    bare = DeviceCorpus.from_arrays(utts, sample_size=150)
    assert bare.frames_flat is None
    got = bare.compute_feature_stats(spec).sums()
    assert got[0] == n and _same_bits(got[1], each.sums()[1]) and \
        _same_bits(got[2], each.sums()[2])
    # a given normaliser is applied the same way
    given = DeviceCorpus.from_arrays(utts, spec=spec, normalize=norm)
    assert _same_bits(given.frames_flat, corpus.frames_flat)
    assert given.normalizer is norm
    # frames from memory
    counts = [-(-u // 16) for u in UTT]
    parts = np.split(raw[0], np.cumsum(counts)[:-1])
    mem = DeviceCorpus.from_arrays(utts, frames=parts, hop=16,
                                   normalize='corpus', normalize_clip=3.0)
    assert _same_bits(mem.frames_flat, corpus.frames_flat)
    assert mem.spec is None and mem.normalizer.entry() == norm.entry()


@pytest.mark.parametrize('lc', ['frames', 'rows'])
def test_corpus_batches_copy_normalised_frames(corpora, lc):
    utts, spec, corpus, twin = corpora
    norm, B = corpus.normalizer, 3
    for step in range(3):
        b, t = corpus.batch(step, B, lc=lc), twin.batch(step, B, lc=lc)
        torch.cuda.synchronize()
        assert _same_bits(b.audio, t.audio) and \
            b.lengths.tolist() == t.lengths.tolist()
        p = twin.plan(step, B)
        if lc == 'frames':
            f_lo, f_hi, off = twin.index.frame_window(p, 16,
                                                      twin.frame_counts)
            assert b.offsets.tolist() == off.tolist()
            got, src, real = b.frames, t.frames.cpu().numpy(), f_hi - f_lo
        else:
            got, src, real = b.rows, t.rows.cpu().numpy(), p.n
        want = np.zeros_like(src)
        for j in range(B):
            want[j, :real[j]] = norm.reference(src[j, :real[j]])
            assert not src[j, real[j]:].any()
        assert _same_bits(got, want)
        assert (want != src).any()


def test_two_shards_get_the_whole_corpus_normaliser(corpora):
    from wavenet import features
    from wavenet.corpus import DeviceCorpus
    utts, spec, corpus, _ = corpora
    shards = [utts[r::2] for r in range(2)]
    vec = [DeviceCorpus.from_arrays(s).compute_feature_stats(spec).vector()
           for s in shards]
    # (a shard's resident frames are summed in one launch, not per utterance:
    # what it hands to the callable is within the bound of that, and the sum
    # over the ranks is what comes back)
    seen = []

    def summed(v):
        seen.append(np.array(v))
        return vec[0] + vec[1]
    got = [DeviceCorpus.from_arrays(s, spec=spec, normalize='corpus',
                                    normalize_clip=3.0, world=2,
                                    stats_allreduce=summed) for s in shards]
    assert len(seen) == 2 and all(v.dtype == np.float64 and
                                  v.shape == (17,) for v in seen)
    for r in range(2):
        assert seen[r][0] == vec[r][0]
        assert np.allclose(seen[r], vec[r], rtol=1e-12)
    want = features.Normalizer.from_stats(
        features.FeatureStats.from_vector(vec[0] + vec[1]), clip=3.0)
    for c in got:
        assert c.normalizer.entry() == want.entry()
        assert c.feature_stats.count == corpus.feature_stats.count
    # ... which is the whole corpus's, to a float32 rounding
    whole = corpus.normalizer
    assert np.allclose(want.shift, whole.shift, rtol=2e-7, atol=0)
    assert np.allclose(want.scale, whole.scale, rtol=2e-7, atol=0)
    with pytest.raises(ValueError, match='stats_allreduce'):
        got[0].compute_feature_stats(spec)


def test_loss_on_the_corpus_normalised_frames(corpora):
    """A tiny LC-upsampler model, scales (4, 4), Lc 8: the loss on the
    corpus's frames is the loss on the twin's frames normalised on the host."""
    from wavenet import WaveNetModel
    utts, spec, corpus, twin = corpora
    B, norm = 3, corpus.normalizer
    net = WaveNetModel(B, [1, 2, 4, 8, 1, 2, 4, 8], 2, 32, 32, 64,
                       quantization_channels=64, use_biases=True, seed=3,
                       local_condition_channels=8,
                       local_condition_upsample_scales=(4, 4))
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        net.params.copy_(0.3 * torch.randn(net.params.shape, generator=g))
    for step in (0, 1):
        b, t = corpus.batch(step, B), twin.batch(step, B)
        loss = float(net.loss(b.audio, local_condition_batch=b.frames,
                              local_condition_offset=b.offsets,
                              lengths=b.lengths))
        p = twin.plan(step, B)
        f_lo, f_hi, _ = twin.index.frame_window(p, 16, twin.frame_counts)
        src = t.frames.cpu().numpy()
        host = np.zeros_like(src)
        for j in range(B):
            host[j, :f_hi[j] - f_lo[j]] = \
                norm.reference(src[j, :f_hi[j] - f_lo[j]])
        ref = float(net.loss(t.audio, local_condition_batch=host,
                             local_condition_offset=t.offsets,
                             lengths=t.lengths))
        raw = float(net.loss(t.audio, local_condition_batch=src,
                             local_condition_offset=t.offsets,
                             lengths=t.lengths))
        assert np.isfinite(loss) and loss == ref, (step, loss, ref)
        assert raw != loss
