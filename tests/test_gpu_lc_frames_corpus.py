"""DeviceCorpus with a mel + F0 front end (wavenet/frontend.py) and
normalize='corpus': the resident frames are the front end's of every whole
utterance with the corpus's normaliser, bit for bit; the statistics are those
of the raw mel channels (compute_feature_stats: an n_mels-channel
FeatureStats); and a batch's frames under history and context are the
whole-utterance rows of their place."""
import numpy as np
import pytest
import torch

import lc_frames_ref as R

pytestmark = pytest.mark.gpu

HOP, MELS = 16, 8


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope='module')
def built(hip_lib):
    """(corpus, spec, utterances, whole): three short clips, the composite
    spec, and spec-with-the-corpus's-normaliser of every whole utterance --
    computed once and left unchanged."""
    from wavenet import features, frontend, pitch
    from wavenet.corpus import DeviceCorpus
    utts = [R.tone_with_gap(f, n, gap, seed=i) for i, (f, n, gap) in
            enumerate(((150.0, 1500, (400, 700)), (240.0, 1000, (0, 200)),
                       (330.0, 1237, (900, 1237))))]
    mel = features.MelSpec(16000, n_fft=64, hop=HOP, n_mels=MELS)
    t = pitch.PitchTracker(16000, hop=HOP, fmin=100.0, window=128)
    spec = frontend.MelPitchSpec(mel, t, None, True)
    corpus = DeviceCorpus.from_arrays(utts, spec=spec, normalize='corpus',
                                      normalize_clip=3.0, sample_size=300,
                                      history=70, seed=3)
    whole = [spec.with_normalizer(corpus.normalizer)(u) for u in utts]
    return corpus, spec, utts, whole


def test_resident_frames_are_the_front_ends(built):
    from wavenet import features
    corpus, spec, utts, whole = built
    L = MELS + 2
    assert corpus.Lc == L and corpus.hop == HOP
    assert corpus.frame_counts.tolist() == [-(-u.shape[0] // HOP)
                                            for u in utts]
    assert isinstance(corpus.normalizer, features.Normalizer)
    assert corpus.normalizer.n_channels == MELS
    assert corpus.spec.normalizer is corpus.normalizer
    assert corpus.spec.channels == L and corpus.spec.tracker is spec.tracker
    resident = corpus.frames_flat.view(-1, L)
    assert resident.shape[0] == int(corpus.frame_counts.sum())
    o = 0
    for u, w in enumerate(whole):
        F = w.shape[0]
        assert torch.equal(_bits(resident[o:o + F]), _bits(w)), u
        o += F
    # the pitch channels were not normalised: in [0, 1], the flag 0 or 1,
    # both kinds of frame present
    flag = resident[:, L - 1]
    assert bool(((flag == 0) | (flag == 1)).all())
    assert 0 < int(flag.sum()) < flag.shape[0]
    f0ch = resident[:, L - 2]
    assert bool(((f0ch >= 0) & (f0ch <= 1)).all())
    # ... and the mel channels were clamped by the clip
    assert float(resident[:, :MELS].abs().max()) <= 3.0


def test_statistics_are_the_raw_mel_channels(built):
    from wavenet import features
    corpus, spec, utts, _ = built
    got = corpus.feature_stats
    want = corpus.compute_feature_stats(spec)
    assert got.n_channels == want.n_channels == MELS
    a, b = got.sums(), want.sums()
    assert a[0] == b[0] == int(corpus.frame_counts.sum())
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    # interchangeable with a mel run's: the mel part alone sums the same
    mel_only = corpus.compute_feature_stats(spec.mel)
    c = mel_only.sums()
    assert np.array_equal(a[1], c[1]) and np.array_equal(a[2], c[2])
    norm = features.Normalizer.from_stats(got, 3.0)
    assert np.array_equal(norm.shift, corpus.normalizer.shift)
    assert np.array_equal(norm.scale, corpus.normalizer.scale)


def test_batch_frames_are_the_whole_utterance_rows(built):
    from wavenet.corpus import window_frames
    corpus, spec, utts, whole = built
    B, L = 4, MELS + 2
    seen_history = False
    for step in range(4):
        p = corpus.plan(step, B)
        b = corpus.batch(step, B)
        f_lo, f_hi, off = corpus.index.frame_window(p, HOP,
                                                    corpus.frame_counts)
        assert b.frames.shape == (B, window_frames(p.T, HOP), L)
        assert b.offsets.tolist() == off.tolist()
        seen_history = seen_history or bool(np.asarray(b.history).any())
        for k in range(B):
            n = int(f_hi[k] - f_lo[k])
            want = whole[int(p.utt[k])][int(f_lo[k]):int(f_hi[k])]
            assert torch.equal(_bits(b.frames[k, :n]), _bits(want)), (step, k)
            assert not bool(_bits(b.frames[k, n:]).any())
    assert seen_history
