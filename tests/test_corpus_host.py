"""The device-resident corpus without a GPU: CorpusIndex against the
independent restatement (tests/corpus_ref.py), the order's properties, rank
shards, errors before any library or device is touched, train.py's flag
errors, argument validation of the two entry points."""
import ctypes
import os
import sys

import numpy as np
import pytest
from scipy.io import wavfile

import corpus_ref as R
from util import ROOT

sys.path.insert(0, ROOT)

SIZE = 10
LENGTHS = [1, SIZE - 1, SIZE, SIZE + 1, 3 * SIZE + 7]
IDS = [3, 1, 4, 1, 5]


def _index(crop='pieces', size=SIZE, seed=7, lengths=LENGTHS, ids=IDS):
    from wavenet.corpus import CorpusIndex
    return CorpusIndex(lengths, ids, size, crop, seed)


def _slots(p):
    return [(int(u), int(s), int(n), None if p.gc is None else int(p.gc[j]))
            for j, (u, s, n) in enumerate(zip(p.utt, p.start, p.n))]


def _no_library(monkeypatch):
    from wavenet import _lib
    monkeypatch.setattr(_lib, 'load', lambda: pytest.fail('library touched'))
    monkeypatch.setattr(_lib, 'require_gpu',
                        lambda: pytest.fail('device touched'))


def test_splitmix64_restatements_agree():
    from wavenet import corpus
    xs = [0, 1, 12345, (1 << 64) - 1, 0x9E3779B97F4A7C15]
    want = [R.splitmix64_int(x) for x in xs]
    assert [int(v) for v in R.splitmix64(np.array(xs, np.uint64))] == want
    assert [int(v) for v in corpus.splitmix64(np.array(xs, np.uint64))] == want
    # (splitmix64's published first output for state 0)
    assert want[0] == 0xE220A8397B1DCDAF
    assert int(corpus.draw_bits(5, np.array([9], np.uint64))[0]) == \
        R.splitmix64_int(5 ^ R.splitmix64_int(9))


@pytest.mark.parametrize('crop, size', [('pieces', SIZE), ('pieces', None),
                                        ('random', SIZE)])
def test_index_equals_restatement(crop, size, monkeypatch):
    _no_library(monkeypatch)
    ix = _index(crop, size)
    items = R.make_items(LENGTHS, size, crop)
    assert ix.P == len(items) == len(ix)
    assert [tuple(r) for r in ix.items.tolist()] == items
    # (P = 9 pieces or 5 items: B = 4 and 7 divide neither; the batches
    # straddle epoch boundaries, B = 7 > P = 5 straddles every time)
    for B in (1, 4, 7):
        assert ix.P % B or B == 1
        straddled = False
        for step in range(9):
            p = ix.plan(step, B)
            slots, T = R.plan(LENGTHS, size, crop, 7, step, B, IDS)
            assert _slots(p) == slots, (crop, size, B, step)
            assert p.T == T == max(s[2] for s in slots)
            assert p.n.dtype == np.int64 and p.gc.dtype == np.int32
            e0, nE = ix.epochs(step, B)
            assert e0 == ix.epoch_of(step, B) == step * B // ix.P
            straddled |= nE > 1
            # a given T cuts n
            cut, Tc = R.plan(LENGTHS, size, crop, 7, step, B, IDS, T=3)
            pc = ix.plan(step, B, T=3)
            assert _slots(pc) == cut and pc.T == Tc == 3
        assert straddled or B == 1


def test_pieces_are_the_readers_cut():
    ix = _index('pieces', SIZE)
    got = {}
    for u, k in ix.items.tolist():
        got.setdefault(u, []).append(k)
    for u, n in enumerate(LENGTHS):
        assert got[u] == list(range(0, n, SIZE))
    p = ix.plan(0, ix.P)
    assert sorted(p.n.tolist()) == sorted(
        min(SIZE, n - k) for u, n in enumerate(LENGTHS)
        for k in range(0, n, SIZE))


def test_every_epoch_is_a_permutation_and_epochs_differ():
    ix = _index('pieces', SIZE)
    perms = [ix.perm(e).tolist() for e in range(4)]
    for e, pm in enumerate(perms):
        assert sorted(pm) == list(range(ix.P))
        assert pm == R.permutation(7, e, ix.P)
    assert len(set(map(tuple, perms))) == 4
    # one epoch of batches visits every item once, whatever B
    for B in (1, 3, 9):
        seen = []
        for step in range(-(-2 * ix.P // B)):
            p = ix.plan(step, B)
            seen += list(zip(p.utt.tolist(), p.start.tolist()))
        for e in range(2):
            assert sorted(seen[e * ix.P:(e + 1) * ix.P]) == \
                sorted(map(tuple, ix.items.tolist()))
    assert _index(seed=8).perm(0).tolist() != perms[0]


def test_seed_and_step_reproduce_and_a_resumed_run_continues():
    run = [_slots(_index('random').plan(k, 3)) for k in range(12)]
    ix = _index('random')
    assert [_slots(ix.plan(k, 3)) for k in range(12)] == run
    for k in (0, 5, 11):
        assert _slots(_index('random').plan(k, 3)) == run[k]   # fresh object
    assert [_slots(_index('random', seed=8).plan(k, 3))
            for k in range(12)] != run


def test_random_starts_in_range_and_vary_between_epochs():
    ix = _index('random')
    assert ix.P == len(LENGTHS)
    starts = {}
    for step in range(40):                   # 40 epochs at B = P
        p = ix.plan(step, ix.P)
        assert sorted(p.utt.tolist()) == list(range(ix.P))
        for u, s, n in zip(p.utt.tolist(), p.start.tolist(), p.n.tolist()):
            nu = LENGTHS[u]
            assert n == min(SIZE, nu)
            assert 0 <= s <= max(nu - SIZE, 0)
            starts.setdefault(u, set()).add(s)
    assert starts[0] == starts[1] == starts[2] == {0}
    assert starts[3] == {0, 1}               # n_u = size + 1: two windows
    assert len(starts[4]) > 10               # 28 windows


def test_frame_window_equals_restatement():
    from wavenet import corpus
    rng = np.random.default_rng(0)
    hop = 4
    frames = [rng.standard_normal((-(-n // hop), 3)).astype(np.float32)
              for n in LENGTHS]
    ix = _index('random')
    from wavenet import WaveNetModel
    assert corpus.LC_CONTEXT_MAX == WaveNetModel.LC_CONTEXT_MAX == R.M
    for step in range(6):
        p = ix.plan(step, 3)
        slots, T = R.plan(LENGTHS, SIZE, 'random', 7, step, 3, IDS)
        win, offs = R.frame_windows(frames, slots, T, hop)
        f_lo, f_hi, off = ix.frame_window(p, hop, [f.shape[0] for f in frames])
        assert off.tolist() == offs.tolist()
        assert win.shape[1] == corpus.window_frames(T, hop)
        for j in range(3):
            assert f_hi[j] - f_lo[j] <= win.shape[1]
            # the model's selection: position offset + t takes this frame
            for t in range(int(p.n[j])):
                assert (off[j] + t) // hop + f_lo[j] == (p.start[j] + t) // hop


def _wav_tree(d, names, n=3000):
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(1)
    for i, name in enumerate(names):
        x = 0.5 * np.sin(2 * np.pi * 200.0 * (i + 1) * np.arange(n + 100 * i)
                         / 16000.0) + 0.01 * rng.standard_normal(n + 100 * i)
        wavfile.write(os.path.join(d, name), 16000,
                      (x * 32767).astype(np.int16))


def test_rank_shards_are_disjoint_and_cover_the_files(tmp_path):
    from wavenet import audio_reader as ar, corpus
    names = ['p%d_%03d.wav' % (225 + i % 3, i) for i in range(7)]
    _wav_tree(str(tmp_path), names)
    files = ar.find_files(str(tmp_path))
    for world in (1, 2, 3, 8):
        shards = [corpus.shard(files, r, world) for r in range(world)]
        assert sorted(sum(shards, [])) == files
        assert sum(len(s) for s in shards) == len(files)
        for r in range(world):        # the reader's own rule
            assert shards[r] == (files[r::world] if world > 1 else files)


def test_index_errors():
    from wavenet.corpus import CorpusIndex
    with pytest.raises(ValueError, match='no items'):
        CorpusIndex([0, 0])
    with pytest.raises(ValueError, match='no items'):
        CorpusIndex([], None, 4)
    with pytest.raises(ValueError, match='sample_size'):
        CorpusIndex([5], crop='random')
    with pytest.raises(ValueError, match='crop'):
        CorpusIndex([5], crop='centre')
    for bad in (0, -4, 2.5, True):
        with pytest.raises(ValueError, match='sample_size'):
            CorpusIndex([5], sample_size=bad)
    with pytest.raises(ValueError, match='seed'):
        CorpusIndex([5], seed=-1)
    with pytest.raises(ValueError, match='lengths'):
        CorpusIndex([5, -1])
    with pytest.raises(ValueError, match='category_ids'):
        CorpusIndex([5, 6], [1])
    ix = CorpusIndex([0, 5, 0, 6], [9, 8, 7, 6], 4)
    assert sorted(set(ix.items[:, 0].tolist())) == [1, 3]   # silent ones dropped
    for bad in ((-1, 2), (0, 0), (0.5, 2)):
        with pytest.raises(ValueError, match='plan'):
            ix.plan(*bad)


def test_device_corpus_errors_come_before_library_and_device(tmp_path,
                                                             monkeypatch,
                                                             capsys):
    _no_library(monkeypatch)
    from wavenet.corpus import DeviceCorpus
    a = [np.zeros(40, np.float32), np.ones(9, np.float32)]
    with pytest.raises(ValueError, match='float32'):
        DeviceCorpus.from_arrays([np.zeros(4)])
    with pytest.raises(ValueError, match='no utterances'):
        DeviceCorpus.from_arrays([])
    with pytest.raises(ValueError, match='sample_size'):
        DeviceCorpus.from_arrays(a, crop='random')
    with pytest.raises(ValueError, match='hop'):
        DeviceCorpus.from_arrays(a, frames=[np.zeros((10, 2), np.float32)] * 2)
    with pytest.raises(ValueError, match='F_u'):
        DeviceCorpus.from_arrays(a, hop=4, frames=[
            np.zeros((9, 2), np.float32), np.zeros((3, 2), np.float32)])
    with pytest.raises(MemoryError) as e:
        DeviceCorpus.from_arrays(a, max_bytes=100)
    assert '196' in str(e.value) and '100' in str(e.value)   # both sizes
    with pytest.raises(ValueError, match='max_bytes'):
        DeviceCorpus.from_arrays(a, max_bytes=0)
    # the directory loader
    d = str(tmp_path / 'wavs')
    with pytest.raises(ValueError, match='No audio files'):
        os.makedirs(d)
        DeviceCorpus(d, 16000, False)
    _wav_tree(d, ['p225_001.wav', 'p226_002.wav', 'clip.wav'])
    with pytest.raises(ValueError, match='pattern having id'):
        DeviceCorpus(d, 16000, True)
    with pytest.raises(ValueError, match='rank'):
        DeviceCorpus(d, 16000, False, rank=2, world=2)
    with pytest.raises(ValueError, match='sample_size'):
        DeviceCorpus(d, 16000, False, crop='random')
    with pytest.raises(ValueError, match='spec'):
        DeviceCorpus(d, 16000, False, spec='mel')
    with pytest.raises(MemoryError) as e:
        DeviceCorpus(d, 16000, False, max_bytes=1000)
    # (clip.wav, 3200 samples, crosses the limit: a lower bound, said as one)
    assert 'at least 12800 bytes' in str(e.value) and \
        'after 1 of its 3 files' in str(e.value) and '1000' in str(e.value)
    # an all-silent directory fails at once, with the reader's warning
    with pytest.raises(ValueError, match='trims to nothing'):
        DeviceCorpus(d, 16000, False, silence_threshold=0.99)
    assert 'contains only silence' in capsys.readouterr().out


# ------------------------------------------------------------ command line
def _argparse_error(capsys, argv):
    import train
    with pytest.raises(SystemExit) as e:
        train.get_arguments(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_train_flag_errors_name_the_flag(capsys):
    import train
    dc = ['--device_corpus', 'true']
    err = _argparse_error(capsys, dc)
    assert '--device_corpus' in err and '--data_dir' in err
    err = _argparse_error(capsys, dc + ['--data_dir', 'x', '--synthetic'])
    assert '--device_corpus' in err and '--synthetic' in err
    err = _argparse_error(capsys, dc + ['--data_dir', 'x', '--lc_channels',
                                        '8', '--lc_hop', '16'])
    assert '--device_corpus' in err and '--lc_features mel' in err
    err = _argparse_error(capsys, ['--crop', 'random'])
    assert '--crop' in err and '--device_corpus' in err
    err = _argparse_error(capsys, dc + ['--data_dir', 'x', '--crop', 'random',
                                        '--sample_size', '0'])
    assert '--crop random' in err and '--sample_size' in err
    err = _argparse_error(capsys, dc + ['--data_dir', 'x', '--crop', 'middle'])
    assert '--crop' in err
    mel = ['--lc_features', 'mel', '--lc_channels', '8', '--lc_hop', '16']
    err = _argparse_error(capsys, mel + ['--lc_feature_context', 'utterance'])
    assert '--lc_feature_context' in err and '--device_corpus' in err
    err = _argparse_error(capsys, dc + ['--data_dir', 'x',
                                        '--lc_feature_context', 'utterance'])
    assert '--lc_feature_context' in err and '--lc_features mel' in err
    err = _argparse_error(capsys, ['--lc_feature_context', 'piece'])
    assert '--lc_feature_context' in err and '--lc_features' in err
    # what parses
    # (an abbreviation argparse accepts counts as given)
    assert train.get_arguments(dc + ['--data_d', 'x']).data_dir == 'x'
    assert train.get_arguments([]).data_dir == train.DATA_DIRECTORY
    a = train.get_arguments(dc + ['--data_dir=x', '--crop', 'random'] + mel +
                            ['--lc_feature_context', 'utterance'])
    assert a.device_corpus and a.crop == 'random' and \
        a.lc_feature_context == 'utterance'
    a = train.get_arguments(mel + ['--lc_feature_context', 'piece'])
    assert a.lc_feature_context == 'piece' and not a.device_corpus
    # without the flags nothing changes
    a = train.get_arguments([])
    assert a.device_corpus is False and a.crop is None and \
        a.lc_feature_context is None


def test_a_restored_training_goes_on_with_the_next_batch(capsys):
    import train
    entry = dict(crop='pieces', seed=0, sample_size=2000,
                 lc_feature_context='piece')
    assert train.corpus_first_batch(None, entry) == 0
    assert capsys.readouterr().out == ''
    assert train.corpus_first_batch(dict(entry, batch=2), entry) == 3
    assert 'continue at 3' in capsys.readouterr().out
    assert train.corpus_first_batch(dict(entry), entry) == 0
    for other in (dict(crop='random'), dict(seed=1), dict(sample_size=None),
                  dict(lc_feature_context='utterance')):
        assert train.corpus_first_batch(dict(entry, batch=2, **other),
                                        entry) == 0
        assert 'starts again' in capsys.readouterr().out


# -------------------------------------------------------------------- ABI
def test_entry_points_validate_without_gpu(hip_lib):
    """wn_corpus_gather / _gather_frames: error codes before any launch; the
    size query needs no device."""
    from wavenet import corpus
    lib = hip_lib
    for T, hop, m in ((1, 1, 0), (64, 4, 8), (16000, 256, 8), (17, 10, 8),
                      (5, 7, 2)):
        assert lib.wn_corpus_window_frames(T, hop, m) == \
            corpus.window_frames(T, hop, m) == R.window_frames(T, hop, m)
    for bad in ((0, 4, 8), (8, 0, 8), (8, 4, -1)):
        assert lib.wn_corpus_window_frames(*bad) == -1
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    assert a % 8 == 0
    a += (16 - a % 16) % 16

    def gather(flat=a, N=64, uo=a, ul=a, U=1, iu=a, is_=a, P=1, perm=a, e0=0,
               nE=1, g0=0, size=0, rnd=0, seed=0, out=a, B=1, T=4):
        return lib.wn_corpus_gather(flat, N, uo, ul, U, iu, is_, P, perm, e0,
                                    nE, g0, size, rnd, seed, out, B, T, None)

    def frames(fr=a, NF=64, fo=a, fl=a, uo=a, ul=a, U=1, iu=a, is_=a, P=1,
               perm=a, e0=0, nE=1, g0=0, size=0, rnd=0, seed=0, hop=4, ctx=8,
               Lc=2, out=a, Fw=18, rows=a, B=1, T=4):
        return lib.wn_corpus_gather_frames(
            fr, NF, fo, fl, uo, ul, U, iu, is_, P, perm, e0, nE, g0, size,
            rnd, seed, hop, ctx, Lc, out, Fw, rows, B, T, None)

    for fn in (gather, frames):
        for name in ('uo', 'ul', 'iu', 'is_', 'perm'):
            assert fn(**{name: None}) == -5, name
        for kw in (dict(B=0), dict(T=0), dict(P=0), dict(B=-1), dict(T=-3),
                   dict(P=-1), dict(U=0), dict(nE=0), dict(size=-1),
                   dict(rnd=1, size=0), dict(g0=-1), dict(e0=1),
                   dict(g0=1), dict(B=2)):
            # (g0 = 1, B = 2 with P = 1, nE = 1: an epoch outside the tables)
            assert fn(**kw) == -1, kw
        assert fn(out=a + 4) == -3
        assert fn(uo=a + 4) == -3
        assert fn(perm=a + 2) == -3
    assert gather(flat=None) == -5 and gather(out=None) == -5
    assert gather(N=0) == -1
    assert gather(flat=a + 4) == -3
    assert frames(fr=None) == -5 and frames(fo=None) == -5 and \
        frames(fl=None) == -5
    assert frames(out=None, rows=None) == -5
    for kw in (dict(hop=0), dict(ctx=-1), dict(Lc=0), dict(Fw=0), dict(NF=0)):
        assert frames(**kw) == -1, kw
    assert frames(fr=a + 4) == -3 and frames(rows=a + 8) == -3 and \
        frames(fo=a + 4) == -3
