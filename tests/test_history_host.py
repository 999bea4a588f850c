"""Piece history without a GPU: WaveNetModel.receptive_field against the
float64 oracle, the argument checks of `history` before any library or device
is touched, the new entry points' argument validation, CorpusIndex(history=)
against tests/hist_ref.py, ValidationSet(history=), the data-parallel
denominator, and the command lines' argparse errors."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import hist_ref
from util import O, ROOT, TINY, cfg_with

sys.path.insert(0, ROOT)


def _net(**kw):
    from wavenet import WaveNetModel
    args = dict(batch_size=3, dilations=[1, 2, 4, 8], filter_width=2,
                residual_channels=32, dilation_channels=32, skip_channels=64,
                quantization_channels=256, use_biases=True, device='cpu')
    args.update(kw)
    return WaveNetModel(**args)


# ---- receptive field ---------------------------------------------------------
def test_receptive_field_of_the_default_model():
    net = _net(dilations=[2 ** i for i in range(10)] * 5, skip_channels=512)
    assert net.receptive_field == 5117
    # the common shape of tests/test_gpu_history.py
    assert _net(dilations=[1, 2, 4, 8, 1, 2, 4, 8]).receptive_field == 32
    assert _net(dilations=[1, 2, 4], filter_width=3).receptive_field == 25


@pytest.mark.parametrize('fw, scalar', [(2, False), (3, False), (4, False),
                                        (2, True)],
                         ids=['k2', 'k3', 'k4', 'scalar_k0_5'])
def test_receptive_field_is_the_oracles(fw, scalar):
    """The float64 oracle's logits row t change when sample t - R + 1
    changes and do not change when any earlier sample does."""
    dil = [1, 2, 4]
    cfg = cfg_with(TINY, dilations=dil, filter_width=fw, batch_size=1,
                   scalar_input=scalar, initial_filter_width=5)
    R = _net(batch_size=1, dilations=dil, filter_width=fw,
             scalar_input=scalar, initial_filter_width=5).receptive_field
    var = O.create_variables(cfg, seed=1, dtype=np.float64, bias_scale=0.1)
    T = R + 6
    a = np.random.default_rng(0).uniform(-1, 1, (1, T)).astype(np.float32)

    def logits(x):
        return O.loss(cfg, var, x, None, None, np.float64,
                      keep=True)[1]['logits'][0]
    base = logits(a)
    for t in (T - 1, T - 3):
        for s in range(t - R + 2):
            b = a.copy()
            # (another mu-law code, another float)
            b[0, s] = -b[0, s] if abs(b[0, s]) > 0.2 else 0.9
            moved = np.abs(logits(b)[t] - base[t]).max()
            if s == t - R + 1:
                assert moved > 0, (t, s)
            else:
                assert moved == 0, (t, s, moved)


# ---- arguments ---------------------------------------------------------------
def test_keyword_only_and_default_none():
    from wavenet import WaveNetModel
    for fn in (WaveNetModel.loss, WaveNetModel.loss_from_codes,
               WaveNetModel.score, WaveNetModel.score_from_codes):
        p = inspect.signature(fn).parameters['history']
        assert p.kind == p.KEYWORD_ONLY and p.default is None, fn


T = 10
BAD = [
    (dict(history=-1), r'\[0, n'),                                # negative
    (dict(history=[0, -2, 0]), r'\[0, n'),
    (dict(history=11), r'\[0, n'),                                # > n = T
    (dict(history=[0, 6, 0], lengths=[10, 5, 3]), r'\[0, n'),     # > n[b]
    (dict(history=torch.tensor([0, 0, 4]), lengths=[10, 5, 3]), r'\[0, n'),
    (dict(history=[1, 2]), 'shape'),                              # B = 3
    (dict(history=[[1, 2, 3]]), 'shape'),
    (dict(history=True), 'integer'),
    (dict(history=[True, False, True]), 'integer'),
    (dict(history=2.0), 'integer'),
    (dict(history=[1.0, 2.0, 3.0]), 'integer'),
    (dict(history=np.array([1, 2, 3], np.float32)), 'integer'),
    (dict(history='rf'), 'integer'),
    (dict(history=10), 'no sample to predict'),                   # all h == n
    (dict(history=[10, 5, 3], lengths=[10, 5, 3]), 'no sample to predict'),
]


@pytest.mark.parametrize('kw, what', BAD, ids=[str(i) for i in range(len(BAD))])
def test_bad_history_raises_before_library_or_device(kw, what, monkeypatch):
    from wavenet import _lib
    net = _net()
    net._check_supported = lambda: None    # (a CPU model: stop before launches)
    monkeypatch.setattr(_lib, 'load', lambda: pytest.fail('library touched'))
    monkeypatch.setattr(_lib, 'require_gpu',
                        lambda: pytest.fail('device touched'))
    codes = torch.zeros((3, T), dtype=torch.int32)
    with pytest.raises(ValueError, match=what):
        net.loss(np.zeros((3, T), np.float32), **kw)
    with pytest.raises(ValueError, match=what):
        net.loss_from_codes(codes, **kw)
    with pytest.raises(ValueError, match=what):
        net.score(np.zeros((3, T), np.float32), **kw)
    with pytest.raises(ValueError, match=what):
        net.score_from_codes(codes, **kw)


def test_check_history_accepts():
    from wavenet.model import check_history, check_lengths
    assert check_history(None, None, None, 3, T, 'loss') == (None, None)
    mask = check_lengths([10, 5, 3], None, 3, T, 'loss')
    assert check_history(None, mask, None, 3, T, 'loss') == (mask, None)
    for ok in (2, np.int64(2), [2, 2, 2], np.array([2, 2, 2], np.uint8),
               torch.tensor([2, 2, 2]), torch.tensor(2)):
        (n, den), h = check_history(ok, mask, None, 3, T, 'loss')
        assert n.dtype == np.int32 and n.tolist() == [10, 5, 3]
        assert h.dtype == np.int32 and h.tolist() == [2, 2, 2] and den == 12.0
    # without lengths every clip has T samples
    (n, den), h = check_history([0, 10, 4], None, None, 3, T, 'loss')
    assert n.tolist() == [T] * 3 and h.tolist() == [0, 10, 4] and den == 16.0
    # loss_denominator still overrides, also where this rank has no target
    mask = check_lengths([10, 5, 3], 7.5, 3, T, 'loss')
    assert check_history(1, mask, 7.5, 3, T, 'loss')[0][1] == 7.5
    assert check_history([10, 5, 3], mask, 7.5, 3, T, 'loss')[0][1] == 7.5


# ---- entry points ------------------------------------------------------------
def test_window_entries_validate_arguments(hip_lib):
    lib = hip_lib
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    p16 = p + (-p) % 16
    call = lambda logits=p16, ld=256, q=p16, h=p16, n=p16, inv=p16, dl=p16, \
        parts=p16, B=2, T=3, Q=256: lib.wn_xent_window(
            logits, ld, q, h, n, inv, dl, parts, B, T, Q, 1, None)
    for name in ('logits', 'q', 'h', 'n', 'inv', 'parts'):
        assert call(**{name: None}) == -5, name          # WN_ERR_NULL
    for name in ('B', 'T', 'Q'):
        assert call(**{name: 0}) == -1, name             # WN_ERR_BAD_SHAPE
        assert call(**{name: -4}) == -1, name
    assert call(Q=254) == -2 and call(ld=258) == -2      # WN_ERR_UNSUPPORTED
    assert call(logits=p16 + 4) == -3                    # WN_ERR_MISALIGNED
    assert call(dl=p16 + 8) == -3
    assert call(h=p16 + 2) == -3 and call(n=p16 + 2) == -3
    assert call(inv=p16 + 1) == -3
    score = lambda logits=p16, ld=256, q=p16, h=p16, n=p16, row=p16, nll=p16, \
        cnt=p16, hit=p16, scr=p16, B=2, T=3, Q=256: lib.wn_xent_score_window(
            logits, ld, q, h, n, row, nll, cnt, hit, scr, B, T, Q, None)
    for name in ('logits', 'q', 'nll', 'cnt', 'hit', 'scr'):
        assert score(**{name: None}) == -5, name
    assert score(B=0) == -1 and score(ld=128) == -1 and score(Q=254) == -2
    assert score(h=p16 + 2) == -3 and score(nll=p16 + 4) == -3
    # the gathers: history < 0 is a shape error, hist / lens are required
    i64 = (ctypes.c_int64 * 8)()
    t = ctypes.addressof(i64)
    gather = lambda H=0, hist=p16, lens=p16: lib.wn_corpus_gather_hist(
        p16, 64, t, p16, 1, p16, p16, 1, p16, 0, 1, 0, 0, 0, 0, H, p16, hist,
        lens, 1, 4, None)
    assert gather(H=-1) == -1
    assert gather(hist=None) == -5 and gather(lens=None) == -5
    assert gather(hist=p16 + 2) == -3
    assert lib.wn_corpus_gather_frames_hist(
        p16, 64, t, p16, t, p16, 1, p16, p16, 1, p16, 0, 1, 0, 0, 0, 0, -3,
        4, 0, 2, p16, 4, None, 1, 4, None) == -1


# ---- the plan ----------------------------------------------------------------
LENGTHS = [150, 7, 64, 201, 1, 65, 0, 90]
IDS = [3, 1, 4, 1, 5, 9, 2, 6]


# (crop 'random' needs a sample_size)
@pytest.mark.parametrize('crop, size', [
    ('pieces', None), ('pieces', 7), ('pieces', 64), ('random', 7),
    ('random', 64)])
def test_plan_with_history_matches_reference(crop, size):
    from wavenet.corpus import CorpusIndex
    base = CorpusIndex(LENGTHS, IDS, size, crop, seed=7)
    for H in (0, 1, 5, 64, 10 ** 6):
        ix = CorpusIndex(LENGTHS, IDS, size, crop, seed=7, history=H)
        assert ix.history == H and ix.P == base.P
        assert np.array_equal(ix.items, base.items)
        for B in (1, 3, 11):
            for step in (0, 1, 5):
                assert np.array_equal(ix.perm(ix.epoch_of(step, B)),
                                      base.perm(base.epoch_of(step, B)))
                p, p0 = ix.plan(step, B), base.plan(step, B)
                slots, hist, Tref, orig = hist_ref.plan(
                    LENGTHS, size, crop, 7, step, B, H, IDS)
                assert p.T == Tref == int(p.n.max())
                assert p.utt.tolist() == [s[0] for s in slots]
                assert p.start.tolist() == [s[1] for s in slots]
                assert p.n.tolist() == [s[2] for s in slots]
                assert p.gc.tolist() == [s[3] for s in slots]
                assert p.history.tolist() == hist
                assert p.history.dtype == np.int64
                # utterance and original start: those of the plain index
                assert np.array_equal(p.utt, p0.utt)
                assert (p.start + p.history).tolist() == orig == \
                    p0.start.tolist()
                assert np.array_equal(p.n - p.history, p0.n)
                if H == 0:
                    assert np.array_equal(p.start, p0.start)
                    assert not p.history.any()
                # a given T below some h: n' and h are cut to it
                for Tc in (3, 40):
                    pc = ix.plan(step, B, T=Tc)
                    sc, hc, _, _ = hist_ref.plan(LENGTHS, size, crop, 7, step,
                                                 B, H, IDS, T=Tc)
                    assert pc.T == Tc
                    assert pc.start.tolist() == [s[1] for s in sc]
                    assert pc.n.tolist() == [s[2] for s in sc]
                    assert pc.history.tolist() == hc
                    assert (pc.history <= pc.n).all()


def test_plan_reaches_every_history_case():
    """The sweep above is not vacuous: first pieces (h = 0), h < H (a start
    below H), h = H, and a T that cuts below h all occur."""
    from wavenet.corpus import CorpusIndex
    ix = CorpusIndex(LENGTHS, IDS, 64, 'pieces', seed=7, history=100)
    h = np.concatenate([ix.plan(s, 4).history for s in range(6)])
    start = np.concatenate([ix.plan(s, 4).start for s in range(6)])
    assert (h == 0).any() and (h == 64).any() and (h == 100).any()
    assert (start[h < 100] == 0).all()
    cut = ix.plan(0, 12, T=40)
    assert (cut.history == 40).any() and (cut.n == cut.history).any()


def test_history_argument_of_the_index():
    from wavenet.corpus import CorpusIndex
    for bad in (-1, 1.5, True, '5', 1 << 31):
        with pytest.raises(ValueError, match='history'):
            CorpusIndex([10, 20], history=bad)
    p = CorpusIndex([10, 20], sample_size=4, history=3).plan(0, 2)
    assert p._fields[-1] == 'history'
    from wavenet.corpus import Batch
    assert Batch._fields[-1] == 'history'


def test_frame_window_follows_the_extended_piece():
    from wavenet.corpus import CorpusIndex
    hop, m = 4, 1
    ix = CorpusIndex(LENGTHS, IDS, 64, 'pieces', seed=7, history=10)
    counts = [-(-n // hop) for n in LENGTHS]
    for step in range(4):
        p = ix.plan(step, 5)
        f_lo, f_hi, off = ix.frame_window(p, hop, counts, m)
        for j in range(5):
            s, n = int(p.start[j]), int(p.n[j])
            assert f_lo[j] == max(0, s // hop - m)
            assert f_hi[j] == min(counts[p.utt[j]], (s + n - 1) // hop + 1 + m)
            assert off[j] == s - f_lo[j] * hop


# ---- validation set ----------------------------------------------------------
SIZES = [150, 64, 201]


def _wavs(d):
    rng = np.random.default_rng(0)
    for i, n in enumerate(SIZES):
        a = rng.uniform(-0.9, 0.9, n)
        wavfile.write(os.path.join(d, 'c%02d.wav' % i), 16000,
                      (a * 32767).astype(np.int16))


@pytest.mark.parametrize('H', [0, 1, 64, 100, 10 ** 6])
def test_validation_set_pieces_with_history(tmp_path, H):
    from wavenet import evaluate as ev
    from wavenet import audio_reader as ar
    _wavs(str(tmp_path))
    size = 64
    vs = ev.ValidationSet(str(tmp_path), 16000, sample_size=size, history=H)
    plain = ev.ValidationSet(str(tmp_path), 16000, sample_size=size)
    assert len(vs) == len(plain) == sum(-(-n // size) for n in SIZES)
    want = []
    for f in plain.files:
        audio = ar.load_wav(f, 16000).reshape(-1)
        for lo, hi, h in hist_ref.validation_pieces(audio.size, size, H):
            want.append((audio[lo:hi], h))
    assert vs.piece_history == [h for _, h in want]
    for (piece, _, _, _), (ref, h), (own, _, _, _) in zip(vs.pieces, want,
                                                         plain.pieces):
        assert np.array_equal(piece, ref)
        assert np.array_equal(piece[h:], own)
    # five-tuples appear only for H > 0
    items = list(vs.batches(4))
    assert all(len(it) == (5 if H > 0 else 4) for it in items)
    assert all(len(it) == 4 for it in plain.batches(4))
    if H > 0:
        got = np.concatenate([it[4] for it in items])
        assert got.dtype == np.int64 and got.tolist() == vs.piece_history
        for audio, lengths, _, _, h in items:
            assert (h <= lengths).all() and audio.shape[1] == lengths.max()
        assert sum(int((it[1] - it[4]).sum()) for it in items) == sum(SIZES)


def test_validation_set_history_rows_and_frames(tmp_path):
    """The conditioning follows the extended piece: rows from k - h on, the
    frames' offset moved back by h."""
    from wavenet import evaluate as ev
    _wavs(str(tmp_path))
    hop, Lc, H, size = 4, 3, 10, 64
    rng = np.random.default_rng(1)
    for i, n in enumerate(SIZES):
        np.save(os.path.join(str(tmp_path), 'c%02d.npy' % i),
                rng.standard_normal((-(-n // hop), Lc)).astype(np.float32))
    kw = dict(sample_size=size, lc_channels=Lc, lc_hop=hop)
    for frames in (False, True):
        vs = ev.ValidationSet(str(tmp_path), 16000, lc_frames=frames,
                              history=H, **kw)
        plain = ev.ValidationSet(str(tmp_path), 16000, lc_frames=frames, **kw)
        for (a, _, _, c), h, (a0, _, _, c0) in zip(vs.pieces, vs.piece_history,
                                                   plain.pieces):
            if frames:
                assert c[0] is c0[0] or np.array_equal(c[0], c0[0])
                assert c[1] == c0[1] - h
            else:
                assert c.shape[0] == a.shape[0]
                assert np.array_equal(c[h:], c0)
    with pytest.raises(ValueError, match='history'):
        ev.ValidationSet(str(tmp_path), 16000, history=-1)


def test_totals_hands_history_to_score():
    from wavenet import evaluate as ev
    seen = []

    class Net(object):
        device = torch.device('cpu')
        lc_up = False

        def score(self, audio, gc, **kw):
            seen.append(kw)
            z = torch.zeros(2, dtype=torch.float64)
            from wavenet.scoring import Score
            return Score(z, z.to(torch.int32), z.to(torch.int32), None)

    a, n = np.zeros((2, 5), np.float32), np.array([5, 3])
    ev.totals(Net(), [(a, n, None, None), (a, n, None, None, np.array([2, 1]))])
    assert 'history' not in seen[0]
    assert seen[1]['history'].tolist() == [2, 1]
    # the wrappers pass the fifth item through

    class Emph(object):
        def pre(self, audio, lengths):
            return audio + 1
    out = list(ev.with_emphasis(Emph(), [(a, n, None, None),
                                         (a, n, None, None, np.array([2, 1]))]))
    assert len(out[0]) == 4 and len(out[1]) == 5
    assert out[1][4].tolist() == [2, 1] and float(out[1][0].max()) == 1.0


# ---- data-parallel denominator -------------------------------------------------
def test_masked_denominator_with_history():
    from wavenet import parallel
    assert parallel.masked_denominator([5, 7, 1]) == 13.0
    assert parallel.masked_denominator([5, 7, 1], history=None) == 13.0
    assert parallel.masked_denominator([5, 7, 1], history=[0, 0, 0]) == 13.0
    assert parallel.masked_denominator([5, 7, 1], history=[2, 7, 0]) == 4.0
    assert parallel.masked_denominator(np.array([16000, 9000]),
                                       history=np.array([5117, 0])) == 19883.0
    assert parallel.masked_denominator(torch.tensor([3, 4]), history=3) == 1.0
    assert parallel.masked_denominator([3, 4], 'cpu', history=[3, 4]) == 0.0
    assert hist_ref.denominator([5, 7, 1], [2, 7, 0]) == 4.0


# ---- command lines -------------------------------------------------------------
def test_piece_history_flag_errors(capsys):
    import evaluate
    import train
    for argv, what in (
            (['--piece_history', 'rf'], '--device_corpus true'),
            (['--piece_history', '8', '--data_dir', 'x', '--device_corpus',
              'true', '--sample_size', '0'], '--sample_size'),
            (['--piece_history', '8', '--sample_size', '0'],
             '--device_corpus true and --sample_size'),
            (['--piece_history', '-3', '--data_dir', 'x', '--device_corpus',
              'true'], 'piece_history'),
            (['--piece_history', 'all', '--data_dir', 'x', '--device_corpus',
              'true'], 'piece_history')):
        with pytest.raises(SystemExit):
            train.get_arguments(argv)
        assert what in capsys.readouterr().err, argv
    a = train.get_arguments(['--piece_history', 'rf', '--data_dir', 'x',
                             '--device_corpus', 'true', '--sample_size', '64'])
    assert a.piece_history == 'rf'
    a = train.get_arguments(['--piece_history', '12', '--data_dir', 'x',
                             '--device_corpus', 'true'])
    assert a.piece_history == 12
    assert train.get_arguments([]).piece_history is None
    with pytest.raises(SystemExit):
        evaluate.get_arguments(['ckpt', '--data_dir', 'x', '--piece_history',
                                'rf'])
    assert '--sample_size' in capsys.readouterr().err
    a = evaluate.get_arguments(['ckpt', '--data_dir', 'x', '--sample_size',
                                '64', '--piece_history', 'rf'])
    assert a.piece_history == 'rf'
    from wavenet.cli import piece_history
    params = dict(dilations=[2 ** i for i in range(10)] * 5, filter_width=2,
                  scalar_input=False, initial_filter_width=32)
    assert piece_history('rf', params) == 5117
    assert piece_history(40, params) == 40 and piece_history(None, params) == 0


def test_corpus_settings_and_resume():
    import argparse
    import train
    args = argparse.Namespace(crop=None, sample_size=64,
                              lc_feature_context=None)
    plain = train.corpus_settings(args)
    assert 'history' not in plain                    # absent = 0
    entry = train.corpus_settings(args, 32)
    assert entry['history'] == 32
    assert {k: v for k, v in entry.items() if k != 'history'} == plain
    # a run resumed with another history continues the same sequence
    assert train.corpus_first_batch(dict(plain, batch=6), entry) == 7
    assert train.corpus_first_batch(dict(entry, batch=6), plain) == 7
    assert train.corpus_first_batch(dict(entry, batch=6, crop='random'),
                                    entry) == 0
