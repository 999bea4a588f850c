"""Held-out evaluation without a GPU: wn_xent_score's argument validation,
WaveNetModel.score's argument checks on a bookkeeping-only model, the
validation set's single deterministic pass (wavenet/evaluate.py), evaluate()'s
arithmetic on a stub model, sum_over_ranks over gloo, train.py's flag errors,
and the float64 scoring reference (tests/score_ref.py) against brute force."""
import ctypes
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
from scipy.io import wavfile

import score_dp_worker
import score_ref
from util import ROOT

sys.path.insert(0, ROOT)

T = 10


# ---- the C ABI -------------------------------------------------------------------
def test_wn_xent_score_validates_arguments(hip_lib):
    lib = hip_lib
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    assert a % 16 == 0

    def call(logits=a, ld=256, q=a, lengths=a, row=a, nll=a, cnt=a, cor=a,
             scratch=a, B=2, T=3, Q=256):
        return lib.wn_xent_score(logits, ld, q, lengths, row, nll, cnt, cor,
                                 scratch, B, T, Q, None)
    for name in ('logits', 'q', 'nll', 'cnt', 'cor', 'scratch'):
        assert call(**{name: None}) == -5, name
    for kw in (dict(B=0), dict(T=0), dict(Q=0), dict(B=-1), dict(ld=128)):
        assert call(**kw) == -1, kw
    assert call(Q=254, ld=256) == -2
    assert call(ld=258) == -2
    assert call(logits=a + 4) == -3
    assert call(lengths=a + 2) == -3
    assert call(nll=a + 4) == -3                     # float64: 8 bytes
    assert call(row=a + 1) == -3
    assert call(cnt=a + 2) == -3 and call(cor=a + 2) == -3
    assert lib.wn_xent_score_scratch_floats(8 * 16000) == 2 * 8 * 16000
    assert lib.wn_xent_score_scratch_floats(0) == 0


def test_header_and_binding_table_hold_the_new_entries(hip_lib):
    from wavenet import _lib
    import test_abi
    syms = test_abi.declared_symbols()
    for s in ('wn_xent_score', 'wn_xent_score_scratch_floats'):
        assert s in syms and s in _lib.SIGNATURES and hasattr(hip_lib, s)
    assert sorted(_lib.SIGNATURES) == syms


# ---- WaveNetModel.score's checks -------------------------------------------------
def _net(**kw):
    from wavenet import WaveNetModel
    args = dict(batch_size=3, dilations=[1, 2, 4, 8], filter_width=2,
                residual_channels=32, dilation_channels=32, skip_channels=64,
                quantization_channels=256, use_biases=True, device='cpu')
    args.update(kw)
    net = WaveNetModel(**args)
    net._check_supported = lambda: None   # (a CPU model: stop before launches)
    return net


BAD_LENGTHS = [([10, 5], 'shape'), ([10, 5, 0], r'\[1, T\]'),
               ([10, 5, 11], r'\[1, T\]'), ([1.0, 2.0, 3.0], 'integers'),
               ([True, True, True], 'integers')]


@pytest.mark.parametrize('lengths, what', BAD_LENGTHS,
                         ids=[str(i) for i in range(len(BAD_LENGTHS))])
def test_score_raises_what_loss_raises_for_lengths(lengths, what):
    net = _net()
    audio = np.zeros((3, T), np.float32)
    codes = torch.zeros((3, T), dtype=torch.int32)
    for fn, x in ((net.loss, audio), (net.score, audio),
                  (net.loss_from_codes, codes), (net.score_from_codes, codes)):
        with pytest.raises(ValueError, match=what):
            fn(x, lengths=lengths)


def test_score_checks_the_rows_it_was_given_not_batch_size():
    """A 2-D input of another row count is a batch of that many clips: the
    lengths are checked against ITS rows."""
    net = _net()
    with pytest.raises(ValueError, match=r'shape \[5\]'):
        net.score(np.zeros((5, T), np.float32), lengths=[3, 3, 3])
    with pytest.raises(ValueError, match=r'shape \[2\]'):
        net.score_from_codes(torch.zeros((2, T), dtype=torch.int32),
                             lengths=[3, 3, 3])
    # a 1-D input is reshaped to batch_size rows as loss does
    with pytest.raises(ValueError, match=r'shape \[3\]'):
        net.score(np.zeros(3 * T, np.float32), lengths=[3, 3])


def test_score_local_condition_errors_are_those_of_loss():
    audio = np.zeros((3, T), np.float32)
    plain, lc = _net(), _net(local_condition_channels=4)
    rows = np.zeros((3, T, 4), np.float32)
    for fn in (plain.loss, plain.score):
        with pytest.raises(ValueError, match='built without local'):
            fn(audio, local_condition_batch=rows)
    for fn in (lc.loss, lc.score):
        with pytest.raises(ValueError, match='is required'):
            fn(audio)
        with pytest.raises(ValueError, match=r'\[B, T, Lc\]'):
            fn(audio, local_condition_batch=rows[:, :5])
        with pytest.raises(ValueError, match='local_condition_offset'):
            fn(audio, local_condition_batch=rows, local_condition_offset=3)
    with pytest.raises(TypeError):
        plain.score(audio, None, rows)           # keyword only, as loss's


def test_score_is_documented_against_the_loss():
    from wavenet import WaveNetModel
    doc = WaveNetModel.score.__doc__
    assert 'nll.sum() / sum(n)' in doc and 'count.sum()' in doc


# ---- ValidationSet -----------------------------------------------------------------
SIZES = [5000, 3100, 4200, 2600, 3700]
RATE = 16000


def _corpus(d, lc_channels=None, hop=None, silence=0):
    """p<id>_<rec>.wav files of distinct lengths (optionally behind and in
    front of `silence` zero samples) and their frame features."""
    os.makedirs(str(d), exist_ok=True)
    names = []
    for i, n in enumerate(SIZES):
        t = np.arange(n) / float(RATE)
        a = 0.5 * np.sin(2 * np.pi * (200 + 70 * i) * t + 0.1 * i)
        a = np.concatenate([np.zeros(silence), a, np.zeros(silence)])
        name = os.path.join(str(d), 'p%d_%03d.wav' % (3 + (i * 2) % 5, i))
        wavfile.write(name, RATE, (a * 32767).astype(np.int16))
        if lc_channels:
            frames = (a.size + hop - 1) // hop
            f = np.arange(frames, dtype=np.float32)[:, None] + \
                1000.0 * i + 0.01 * np.arange(lc_channels)[None, :]
            np.save(name[:-4] + '.npy', f.astype(np.float32))
        names.append(name)
    return sorted(names)


def test_validation_set_whole_utterances(tmp_path):
    from wavenet import evaluate as ev
    from wavenet.audio_reader import load_wav, category_id_of
    names = _corpus(tmp_path)
    vs = ev.ValidationSet(str(tmp_path), RATE, gc_enabled=True,
                          gc_cardinality=8)
    assert vs.files == names and len(vs) == len(SIZES)
    got = list(vs.batches(2))
    assert [b[0].shape[0] for b in got] == [2, 2, 1]          # ragged end
    lengths = np.concatenate([b[1] for b in got])
    assert lengths.tolist() == sorted(SIZES)                   # by length
    by_len = {load_wav(f, RATE).shape[0]: f for f in names}
    for audio, n, gc, lc in got:
        assert lc is None and audio.dtype == np.float32
        assert n.dtype == np.int64 and gc.dtype == np.int32
        assert audio.shape == (len(n), n.max())
        for j in range(len(n)):
            f = by_len[int(n[j])]
            assert np.array_equal(audio[j, :n[j]], load_wav(f, RATE))
            assert not audio[j, n[j]:].any()                   # zero padding
            assert gc[j] == category_id_of(f)                  # its own clip's
    # a second pass and a second set give the same batches
    again = list(ev.ValidationSet(str(tmp_path), RATE, gc_enabled=True
                                  ).batches(2))
    for a, b in zip(got, again):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(a[2], b[2])
    with pytest.raises(ValueError, match='gc_cardinality'):
        ev.ValidationSet(str(tmp_path), RATE, gc_enabled=True,
                         gc_cardinality=4)
    with pytest.raises(ValueError, match='No audio files'):
        ev.ValidationSet(str(tmp_path / 'nothing'), RATE)


def test_validation_set_pieces_are_cut_per_file(tmp_path):
    from wavenet import evaluate as ev
    names = _corpus(tmp_path)
    vs = ev.ValidationSet(str(tmp_path), RATE, sample_size=2000)
    sizes = [SIZES[int(f[-7:-4])] for f in names]   # (sorted by speaker id)
    assert sizes != SIZES
    want = []
    for n in sizes:
        want += [min(2000, n - k) for k in range(0, n, 2000)]
    # file order, nothing carried from one file into the next
    assert [p[0].shape[0] for p in vs.pieces] == want
    assert [os.path.basename(p[1]) for p in vs.pieces] == \
        [os.path.basename(f) for f, n in zip(names, sizes)
         for _ in range(0, n, 2000)]
    audio, n, gc, lc = next(vs.batches(4))
    assert gc is None and lc is None and n.tolist() == want[:4]


def test_validation_set_shards_cover_every_file_once(tmp_path):
    from wavenet import evaluate as ev
    names = _corpus(tmp_path)
    seen = []
    for rank in range(3):
        vs = ev.ValidationSet(str(tmp_path), RATE, rank=rank, world=3)
        assert vs.files == names[rank::3]
        seen += vs.files
    assert sorted(seen) == names
    # more ranks than files: an empty shard is a set without batches
    vs = ev.ValidationSet(str(tmp_path), RATE, rank=6, world=7)
    assert len(vs) == 0 and list(vs.batches(2)) == []


def test_validation_set_local_conditioning_rows_and_frames(tmp_path):
    """Silence trimming moves a clip's start: the rows lose the audio's
    samples, the frames mode's offset is the trimmed start plus the piece's
    position."""
    from wavenet import evaluate as ev
    from wavenet.audio_reader import (load_wav, trim_bounds, lc_path_of,
                                      upsample_lc, pad_lc_frames)
    hop, Lc, thr, size = 80, 3, 0.1, 1500
    names = _corpus(tmp_path, Lc, hop, silence=3000)
    rows = ev.ValidationSet(str(tmp_path), RATE, sample_size=size,
                            silence_threshold=thr, lc_channels=Lc, lc_hop=hop)
    frm = ev.ValidationSet(str(tmp_path), RATE, sample_size=size,
                           silence_threshold=thr, lc_channels=Lc, lc_hop=hop,
                           lc_frames=True)
    assert len(rows) == len(frm)
    k_of = {}
    for pr, pf in zip(rows.pieces, frm.pieces):
        f = pr[1]
        assert pf[1] == f and np.array_equal(pr[0], pf[0])
        audio = load_wav(f, RATE)
        lo, hi = trim_bounds(audio, thr)
        assert lo > 0 and hi < audio.size
        k = k_of.get(f, 0)
        k_of[f] = k + size
        n = pr[0].shape[0]
        assert np.array_equal(pr[0], audio[lo + k:lo + k + n])
        feats = np.load(lc_path_of(f))
        up = upsample_lc(feats, hop, audio.size, Lc)
        assert np.array_equal(pr[3], up[lo + k:lo + k + n])
        frames, off = pf[3]
        assert off == lo + k
        assert np.array_equal(frames, pad_lc_frames(feats, hop, audio.size,
                                                    Lc))
        # the frames at the offset ARE the rows
        assert np.array_equal(frames[(off + np.arange(n)) // hop], pr[3])
    audio, n, gc, lc = next(rows.batches(3))
    assert lc.shape == (3, n.max(), Lc) and not lc[2, n[2]:].any()
    audio, n, gc, (fr, off) = next(frm.batches(3))
    assert fr.shape[0] == 3 and fr.shape[2] == Lc and off.dtype == np.int64
    assert off.tolist() == [p[3][1] for p in frm.pieces[:3]]
    with pytest.raises(ValueError, match='lc_hop'):
        ev.ValidationSet(str(tmp_path), RATE, lc_channels=Lc)


# ---- evaluate() ------------------------------------------------------------------
class _StubNet(object):
    device = torch.device('cpu')

    def __init__(self):
        self.calls = []

    def score(self, audio, gc=None, *, local_condition_batch=None,
              local_condition_offset=0, lengths=None, per_sample=False):
        from wavenet.scoring import Score
        self.calls.append((audio, gc, local_condition_batch,
                           local_condition_offset, lengths))
        n = np.asarray(lengths)
        return Score(torch.tensor(0.5 * (n - 1), dtype=torch.float64),
                     torch.tensor(n - 1, dtype=torch.int32),
                     torch.tensor((n - 1) // 4, dtype=torch.int32), None)


def test_evaluate_arithmetic_and_max_batches():
    from wavenet import evaluate as ev
    lens = [np.array([9, 5]), np.array([13, 1, 3]), np.array([21])]
    fr, off = np.zeros((1, 2, 3), np.float32), np.array([7])
    batches = [(np.zeros((2, 9), np.float32), lens[0], None, None),
               (np.zeros((3, 13), np.float32), lens[1], np.array([1, 0, 2]),
                np.zeros((3, 13, 3), np.float32)),
               (np.zeros((1, 21), np.float32), lens[2], None, (fr, off))]
    net = _StubNet()
    res = ev.evaluate(net, iter(batches))
    count = sum(int((n - 1).sum()) for n in lens)
    hits = sum(int(((n - 1) // 4).sum()) for n in lens)
    assert res == {'nll_per_sample': 0.5,
                   'bits_per_sample': 0.5 / math.log(2.0),
                   'accuracy': hits / count, 'samples': count, 'clips': 6}
    assert len(net.calls) == 3
    assert net.calls[1][1].tolist() == [1, 0, 2] and net.calls[1][3] == 0
    assert net.calls[2][2] is fr and net.calls[2][3] is off   # frames, offsets
    net = _StubNet()
    res = ev.evaluate(net, iter(batches), max_batches=2)
    assert len(net.calls) == 2 and res['clips'] == 5
    assert res['samples'] == int((lens[0] - 1).sum() + (lens[1] - 1).sum())
    # nothing scored: no division by zero
    res = ev.evaluate(_StubNet(), iter([]))
    assert res['samples'] == 0 and res['clips'] == 0
    assert math.isnan(res['nll_per_sample']) and math.isnan(res['accuracy'])


def test_parameters_swapped_restores_on_exception():
    from wavenet import evaluate as ev
    net = _net()
    before = net.params.clone()
    other = torch.arange(net.params.numel(), dtype=torch.float32)
    addr = net.params.data_ptr()
    net._gen = net._bgen = 'stale'
    with pytest.raises(RuntimeError, match='inside'):
        with ev.parameters_swapped(net, other):
            assert torch.equal(net.params, other)
            assert net.params.data_ptr() == addr      # launch plans stay valid
            assert net._gen is None and net._bgen is None
            net._gen = 'made inside'
            raise RuntimeError('inside')
    assert torch.equal(net.params, before) and net._gen is None
    assert net.params.data_ptr() == addr
    with pytest.raises(ValueError, match='floats'):
        with ev.parameters_swapped(net, other[:-1]):
            pass


# ---- sum_over_ranks ----------------------------------------------------------------
def test_sum_over_ranks_identity_when_not_initialised():
    from wavenet import evaluate as ev
    t = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)
    assert ev.sum_over_ranks(t, 'cpu') is t


def test_sum_over_ranks_gloo(tmp_path):
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(score_dp_worker.worker, args=(2, port, str(tmp_path)), nprocs=2,
             join=True)
    want = score_dp_worker.totals(0) + score_dp_worker.totals(1)
    for r in range(2):
        got = np.load(str(tmp_path / ('sum%d.npy' % r)))
        assert got.dtype == np.float64 and np.array_equal(got, want)


# ---- train.py's flags --------------------------------------------------------------
@pytest.mark.parametrize('flags, what', [
    (['--validate_ema', 'true', '--validation_dir', 'x'],
     '--validate_ema true needs --ema_decay'),
    (['--validate_every', '2'], '--validate_every needs --validation_dir'),
    (['--validation_batches', '2'],
     '--validation_batches needs --validation_dir'),
    (['--validate_every', '0', '--validation_dir', 'x'], 'must be positive'),
])
def test_train_validation_flag_errors(flags, what, capsys, tmp_path):
    import train
    assert train.main(['--synthetic', '--logdir', str(tmp_path / 'log')]
                      + flags) == 1
    assert what in capsys.readouterr().out
    assert not os.path.exists(str(tmp_path / 'log'))


def test_evaluate_cli_flag_errors(capsys, tmp_path):
    import evaluate
    ckpt = str(tmp_path / 'none.ckpt')
    assert evaluate.main([ckpt, '--data_dir', str(tmp_path), '--lc_channels',
                          '4']) == 1
    assert '--lc_hop' in capsys.readouterr().out
    assert evaluate.main([ckpt, '--data_dir', str(tmp_path), '--gc_channels',
                          '4']) == 1
    assert 'gc_cardinality' in capsys.readouterr().out


# ---- the reference itself ----------------------------------------------------------
def test_score_ref_rows_against_brute_force():
    rng = np.random.default_rng(0)
    B, T_, Q = 3, 7, 8
    x = rng.uniform(-4, 4, (B, T_, Q + 4))
    x[..., Q:] = 1e30
    codes = rng.integers(0, Q, (B, T_))
    codes[0, 3], codes[1, 2] = -1, Q
    x[2, 1, 5] = x[2, 1, 2] = 9.0            # a tie: index 2 wins
    codes[2, 2] = 2
    x[2, 3, 6] = x[2, 3, 1] = 9.0
    codes[2, 4] = 6                           # target on the higher index
    x[0, 0, 3] = np.nan
    lengths = [7, 1, 6]
    r = score_ref.rows(x, codes, lengths, Q)
    for b in range(B):
        for t in range(T_):
            tg = codes[b, t + 1] if t + 1 < lengths[b] else -1
            has = 0 <= tg < Q
            assert r['has'][b, t] == has
            if not has:
                assert r['nll'][b, t] == 0.0 and not r['hit'][b, t]
                continue
            row = x[b, t, :Q]
            want = math.log(sum(math.exp(v) for v in row)) - row[tg]
            if np.isnan(row).any():
                assert np.isnan(r['nll'][b, t]) and not r['hit'][b, t]
            else:
                assert abs(r['nll'][b, t] - want) < 1e-12
                assert r['hit'][b, t] == (int(np.argmax(row)) == tg)
    assert r['hit'][2, 1] and not r['hit'][2, 3]
    nll, count, correct = score_ref.clips(r)
    assert count.tolist() == [5, 0, 5] and np.isnan(nll[0]) and nll[1] == 0.0
