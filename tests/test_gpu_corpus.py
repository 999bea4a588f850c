"""The device-resident corpus on the GPU: the gather kernels against the
numpy restatement (tests/corpus_ref.py) bit for bit at the smallest shapes at
which they can go wrong, the ring's no-alias rule, the frames window through a
model, and train.py --device_corpus end to end."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import corpus_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float('nan')
LENGTHS = [1, 2, 5, 31, 64, 65, 203]
IDS = [2, 0, 1, 3, 1, 0, 2]
SEED = 11


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    return got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _utterances(lengths=LENGTHS, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1, 1, n).astype(np.float32) for n in lengths]


def _odd_layout(lengths):
    """Odd utterance offsets, every utterance between two gaps (the caller
    fills them with NaN): no row of a batch begins at an aligned index."""
    offs, pos = [], 5
    for n in lengths:
        offs.append(pos)
        pos += n + 1
        pos += 1 - pos % 2          # -> odd
    return offs, pos + 8


def _guarded(corpus, utts, offs, total):
    """Move a corpus's utterances to `offs` in a flat buffer of `total`
    samples that is NaN everywhere else (the class itself only concatenates)."""
    flat = np.full(total, NAN, np.float32)
    for o, u in zip(offs, utts):
        flat[o:o + u.shape[0]] = u
    corpus.flat = torch.from_numpy(flat).to(corpus.device)
    corpus._utt_off = torch.tensor(offs, dtype=torch.int64,
                                   device=corpus.device)
    return corpus


def _thrice(corpus, step, B, check, **kw):
    """Batch `step` three times, each checked and then overwritten with NaN:
    the third lands in the first one's memory (a ring of two), which holds NaN
    by then -- whatever the kernel leaves unwritten shows."""
    seen = []
    for _ in range(3):
        b = corpus.batch(step, B, **kw)
        check(b)
        seen.append(b.audio.data_ptr())
        for t in (b.audio, b.frames, b.rows):
            if t is not None:
                t.fill_(NAN)
    assert seen[0] == seen[2] != seen[1]


@pytest.mark.parametrize('crop, size', [('pieces', 64), ('pieces', 50),
                                        ('pieces', None), ('random', 17)])
def test_gather_equals_restatement_bit_for_bit(hip_lib, crop, size):
    from wavenet.corpus import DeviceCorpus
    utts = _utterances()
    kw = dict(sample_size=size, crop=crop, seed=SEED)
    offs, total = _odd_layout(LENGTHS)
    assert all(o % 2 for o in offs)
    # 1. odd offsets, NaN in every gap and in the bands at both ends
    layouts = [(_guarded(DeviceCorpus.from_arrays(utts, IDS, **kw), utts,
                         offs, total), None)]
    assert np.isnan(layouts[0][0].flat[:5].cpu().numpy()).all() and \
        np.isnan(layouts[0][0].flat[-8:].cpu().numpy()).all()
    # 2. the concatenation; NaN in the first and last sample of every
    # utterance of one parity, the others are compared
    for parity in (0, 1):
        poisoned = [u.copy() for u in utts]
        for i, u in enumerate(poisoned):
            if i % 2 == parity:
                u[0] = u[-1] = NAN
        layouts.append((DeviceCorpus.from_arrays(poisoned, IDS, **kw),
                        1 - parity))
    P = len(R.make_items(LENGTHS, size, crop))
    residues = set()
    for B in (1, 3, 8):
        for step in range(0, -(-2 * P // B) + 1):     # two epochs and a bit
            slots, T = R.plan(LENGTHS, size, crop, SEED, step, B, IDS)
            want = R.gather(utts, slots, T)
            for corpus, keep in layouts:
                rows = [j for j, s in enumerate(slots)
                        if keep is None or s[0] % 2 == keep]

                def check(b):
                    assert b.audio.dtype == torch.float32 and \
                        tuple(b.audio.shape) == (B, T)
                    assert b.lengths.tolist() == [s[2] for s in slots]
                    assert b.lengths.dtype == np.int64
                    assert b.gc.tolist() == [s[3] for s in slots]
                    assert b.gc.dtype == np.int32
                    assert b.frames is b.offsets is b.rows is None
                    got = b.audio.cpu().numpy()
                    assert _same_bits(got[rows], want[rows]), \
                        (crop, size, B, step)
                    for j, s in enumerate(slots):     # exact zeros behind n
                        assert not _bits(got[j, s[2]:]).any()
                _thrice(corpus, step, B, check)
            for u, start, n, _ in slots:
                residues.add((offs[u] + start) % 4)
    # (source indices: odd with the pieces' starts, multiples of the size;
    # every residue mod 4 with random starts)
    assert residues == ({0, 1, 2, 3} if crop == 'random' else {1, 3})
    assert layouts[0][0].epoch_of(3, 8) == 24 // P
    assert layouts[0][0].items.tolist() == \
        [list(i) for i in R.make_items(LENGTHS, size, crop)]


def test_a_cut_to_a_common_length(hip_lib):
    """batch(T=...): what data-parallel ranks agree on."""
    from wavenet.corpus import DeviceCorpus
    utts = _utterances()
    corpus = DeviceCorpus.from_arrays(utts, sample_size=64, seed=SEED)
    for step in range(4):
        slots, T = R.plan(LENGTHS, 64, 'pieces', SEED, step, 3, T=30)
        b = corpus.batch(step, 3, T=30)
        assert _same_bits(b.audio, R.gather(utts, slots, 30))
        assert b.lengths.tolist() == [s[2] for s in slots] and b.gc is None


def test_consecutive_batches_do_not_alias(hip_lib):
    from wavenet.corpus import DeviceCorpus
    lengths = [64, 65, 203, 100]
    hop, Lc = 4, 5
    utts = _utterances(lengths)
    rng = np.random.default_rng(3)
    frames = [rng.standard_normal((-(-n // hop), Lc)).astype(np.float32)
              for n in lengths]
    corpus = DeviceCorpus.from_arrays(utts, frames=frames, hop=hop,
                                      sample_size=17, crop='random', seed=SEED)
    for lc in ('frames', 'rows'):
        held = corpus.batch(0, 3, lc=lc)
        mine = [None if t is None else t.cpu().numpy().copy()
                for t in (held.audio, held.frames, held.rows)]
        for k in range(1, 4):
            nxt = corpus.batch(k, 3, lc=lc)
            torch.cuda.synchronize()
            if k == 1:          # batch k + 1 shares nothing with batch k
                for a, b in zip((held.audio, held.frames, held.rows),
                                (nxt.audio, nxt.frames, nxt.rows)):
                    assert (a is None) == (b is None)
                    if a is not None:
                        assert a.shape == b.shape
                        assert a.data_ptr() != b.data_ptr()
                for t, m in zip((held.audio, held.frames, held.rows), mine):
                    assert t is None or _same_bits(t, m)
            if k == 2:          # ... the batch after it takes its memory
                assert nxt.audio.data_ptr() == held.audio.data_ptr()
                assert not _same_bits(held.audio, mine[0])


def test_many_batch_lengths_do_not_grow_the_buffers(hip_lib):
    """Whole utterances of different lengths: nearly every batch has a T of
    its own.  The output buffers hold RING x the largest batch, no more."""
    from wavenet.corpus import DeviceCorpus, window_frames
    hop, Lc, B = 4, 5, 2
    lengths = [40 + 13 * i for i in range(12)]
    utts = _utterances(lengths, 2)
    rng = np.random.default_rng(4)
    frames = [rng.standard_normal((-(-n // hop), Lc)).astype(np.float32)
              for n in lengths]
    corpus = DeviceCorpus.from_arrays(utts, frames=frames, hop=hop, seed=SEED)
    Tmax = max(lengths)
    bound = corpus.RING * 4 * B * (Tmax + window_frames(Tmax, hop) * Lc +
                                   Tmax * Lc)
    seen, sizes = set(), []
    for sweep in range(2):
        for step in range(18):                    # three epochs
            slots, T = R.plan(lengths, None, 'pieces', SEED, step, B)
            seen.add(T)
            for lc in ('frames', 'rows'):
                b = corpus.batch(step, B, lc=lc)
                assert tuple(b.audio.shape) == (B, T) and \
                    b.audio.is_contiguous()
                assert _same_bits(b.audio, R.gather(utts, slots, T))
                if lc == 'rows':
                    assert _same_bits(b.rows,
                                      R.frame_rows(frames, slots, T, hop))
                else:
                    assert _same_bits(
                        b.frames, R.frame_windows(frames, slots, T, hop)[0])
            assert corpus.buffer_bytes() <= bound
        sizes.append(corpus.buffer_bytes())
    assert len(seen) >= 8
    assert sizes[0] == sizes[1]                   # (nothing new the second time)


FRAME_COUNTS = [1, 2, 9, 40]


def _frame_corpus(hop, Lc, size, seed=5, **kw):
    from wavenet.corpus import DeviceCorpus
    lengths = [F * hop - hop // 2 for F in FRAME_COUNTS]
    utts = _utterances(lengths, seed)
    rng = np.random.default_rng(seed + 1)
    frames = [rng.standard_normal((F, Lc)).astype(np.float32)
              for F in FRAME_COUNTS]
    corpus = DeviceCorpus.from_arrays(utts, [0, 1, 0, 1], frames=frames,
                                      hop=hop, sample_size=size,
                                      crop='random', seed=SEED, **kw)
    return corpus, lengths, utts, frames


@pytest.mark.parametrize('hop', [4, 10])
@pytest.mark.parametrize('Lc', [1, 5, 80])
def test_frames_equal_restatement_bit_for_bit(hip_lib, hop, Lc):
    size = 3 * hop + 1
    corpus, lengths, utts, frames = _frame_corpus(hop, Lc, size)
    assert [f.shape[0] for f in frames] == FRAME_COUNTS == \
        [-(-n // hop) for n in lengths]
    clipped = set()
    for B in (1, 3):
        for step in range(0, 12 // B + 1):
            slots, T = R.plan(lengths, size, 'random', SEED, step, B)
            win, offs = R.frame_windows(frames, slots, T, hop)
            rows = R.frame_rows(frames, slots, T, hop)
            audio = R.gather(utts, slots, T)

            def check_frames(b):
                assert _same_bits(b.audio, audio)
                assert _same_bits(b.frames, win), (hop, Lc, B, step)
                assert b.offsets.tolist() == offs.tolist() and b.rows is None
                assert b.offsets.dtype == np.int64

            def check_rows(b):
                assert _same_bits(b.audio, audio)
                assert _same_bits(b.rows, rows), (hop, Lc, B, step)
                assert b.frames is None and b.offsets is None
            _thrice(corpus, step, B, check_frames)       # ('auto': frames)
            _thrice(corpus, step, B, check_rows, lc='rows')
            for (u, start, n, _), off in zip(slots, offs):
                clipped.add((start // hop - R.M < 0,
                             (start + n - 1) // hop + 1 + R.M >
                             FRAME_COUNTS[u]))
    # windows cut at both of the utterance's ends, at one, and at neither
    assert {(True, True), (False, False)} <= clipped and len(clipped) == 3


@pytest.mark.parametrize('scales', [(2, 5), (2, 2)])
def test_window_and_offsets_through_a_model(hip_lib, scales):
    """loss and every gradient with the corpus's frames window and offsets
    are, bit for bit, those with the whole utterances' frames at offset =
    start."""
    from wavenet import WaveNetModel
    hop, Lc, B, size = int(np.prod(scales)), 5, 3, 37
    corpus, lengths, utts, frames = _frame_corpus(hop, Lc, size)
    net = WaveNetModel(B, [1, 2, 4], 2, 32, 32, 64, quantization_channels=64,
                       use_biases=True, seed=3, local_condition_channels=Lc,
                       local_condition_upsample_scales=scales,
                       local_condition_context=2,
                       global_condition_channels=4,
                       global_condition_cardinality=2)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():          # (no zero weights: everything matters)
        net.params.copy_(0.3 * torch.randn(net.params.shape, generator=g))
    short = 0
    for step in range(4):
        slots, T = R.plan(lengths, size, 'random', SEED, step, B, [0, 1, 0, 1])
        b = corpus.batch(step, B)
        gc = torch.from_numpy(b.gc)
        loss = float(net.loss(b.audio, gc, local_condition_batch=b.frames,
                              local_condition_offset=b.offsets,
                              lengths=b.lengths))
        torch.cuda.synchronize()
        grads = net.grads.clone()
        assert np.isfinite(loss) and bool(torch.isfinite(grads).all())
        # the whole utterances' frames, zeros behind each one's own
        need = max((s[1] + T - 1) // hop + 1 for s in slots)
        whole = np.zeros((B, max(need, max(FRAME_COUNTS)), Lc), np.float32)
        for j, s in enumerate(slots):
            whole[j, :FRAME_COUNTS[s[0]]] = frames[s[0]]
        ref = float(net.loss(R.gather(utts, slots, T), gc,
                             local_condition_batch=whole,
                             local_condition_offset=[s[1] for s in slots],
                             lengths=[s[2] for s in slots]))
        torch.cuda.synchronize()
        assert loss == ref, (step, loss, ref)
        assert torch.equal(grads, net.grads), step
        assert bool((grads != 0).any())
        short += sum(s[2] < T for s in slots)
    assert short                   # (padded clips were among them)


# ------------------------------------------------------------- end to end
PARAMS = {"filter_width": 2, "sample_rate": 16000,
          "dilations": [1, 2, 4, 8, 16, 32],
          "residual_channels": 32, "dilation_channels": 32,
          "quantization_channels": 256, "skip_channels": 64,
          "use_biases": True, "scalar_input": False,
          "initial_filter_width": 32, "residual_postproc": False}
SIZE, BATCH = 2000, 3


def _wavs(directory):
    """Eight short clips of different lengths, two speakers; half of them
    begin with near silence that the trimming removes."""
    os.makedirs(directory)
    rng = np.random.default_rng(5)
    for i in range(8):
        n, lead = 2600 + 517 * i, 2048 * (i % 2)
        tone = 0.8 * np.sin(2 * np.pi * 110.0 * (i + 2) * np.arange(n) /
                            16000.0) + 0.05 * rng.standard_normal(n)
        x = np.concatenate([0.001 * rng.standard_normal(lead), tone])
        wavfile.write(os.path.join(directory, 'p%d_%03d.wav' % (1 + i % 2, i)),
                      16000, (np.clip(x, -1, 1) * 32767).astype(np.int16))


def _reader_arrays(directory, threshold=0.3):
    from wavenet import audio_reader as ar
    files = ar.find_files(directory)
    out = []
    for f in files:
        a = ar.load_wav(f, 16000)
        lo, hi = ar.trim_bounds(a, threshold)
        out.append(a[lo:hi])
    return files, out, [ar.category_id_of(f) for f in files]


def _run(argv, seconds=300):
    """One child under its own time limit; a failure ends the test."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py')] + argv,
                       cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=seconds)
    out = p.stdout.decode()
    assert p.returncode == 0, 'train.py %s\n%s' % (' '.join(argv), out)
    return out


def _losses(out):
    return re.findall(r'step (\d+) - loss = ([0-9.]+), .*?(\d+) real', out)


@pytest.fixture(scope='module')
def wav_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp('corpus') / 'wavs')
    _wavs(d)
    return d


def test_flat_audio_is_the_readers_bit_for_bit(hip_lib, wav_dir):
    from wavenet.corpus import DeviceCorpus
    files, arrays, ids = _reader_arrays(wav_dir)
    assert len(files) == 8 and len(set(a.shape[0] for a in arrays)) == 8
    assert any(a.shape[0] % SIZE for a in arrays)
    corpus = DeviceCorpus(wav_dir, 16000, True, sample_size=SIZE,
                          silence_threshold=0.3, seed=4)
    assert corpus.files == files
    assert corpus.gc_category_cardinality == 3
    assert _same_bits(corpus.flat, np.concatenate(arrays))
    lengths = [a.shape[0] for a in arrays]
    assert corpus.items.tolist() == \
        [list(i) for i in R.make_items(lengths, SIZE, 'pieces')]
    slots, T = R.plan(lengths, SIZE, 'pieces', 4, 2, BATCH, ids)
    b = corpus.batch(2, BATCH)
    assert _same_bits(b.audio, R.gather(arrays, slots, T))
    assert b.gc.tolist() == [s[3] for s in slots]
    # rank shards: the reader's, each its own index
    for r in range(2):
        shard = DeviceCorpus(wav_dir, 16000, True, silence_threshold=0.3,
                             rank=r, world=2)
        assert shard.files == files[r::2]
        assert shard.gc_category_cardinality == 3
        assert _same_bits(shard.flat, np.concatenate(arrays[r::2]))


@pytest.fixture(scope='module')
def runs(hip_lib, wav_dir, tmp_path_factory):
    """train.py --device_corpus true twice, once: six steps (`whole`), and
    three steps into `log_b`, left as written."""
    tmp = tmp_path_factory.mktemp('runs')
    params = str(tmp / 'params.json')
    json.dump(PARAMS, open(params, 'w'))
    common = ['--data_dir', wav_dir, '--wavenet_params', params,
              '--device_corpus', 'true', '--mask_padding', 'true',
              '--gc_channels', '4', '--sample_size', str(SIZE),
              '--batch_size', str(BATCH), '--silence_threshold', '0.3']
    log_a, log_b = str(tmp / 'a'), str(tmp / 'b')
    whole = _losses(_run(common + ['--num_steps', '6', '--logdir', log_a]))
    assert [k for k, _, _ in whole] == ['0', '1', '2', '3', '4', '5']
    first = _losses(_run(common + ['--num_steps', '3', '--logdir', log_b]))
    return dict(common=common, whole=whole, first=first, log_a=log_a,
                log_b=log_b)


def test_train_prints_the_losses_of_a_python_loop(runs, wav_dir):
    """train.py --device_corpus true against net.loss + minimize on host
    batches assembled by the restatement; the same lines from a second run."""
    import train
    from wavenet import WaveNetModel, optimizer_factory
    whole = runs['whole']
    assert runs['first'] == whole[:3], (whole, runs['first'])
    ck = torch.load(train.latest_checkpoint(runs['log_a']),
                    map_location='cpu')
    assert ck['device_corpus'] == dict(crop='pieces', seed=train.CORPUS_SEED,
                                       sample_size=SIZE,
                                       lc_feature_context='piece', batch=5)
    _, arrays, ids = _reader_arrays(wav_dir)
    lengths = [a.shape[0] for a in arrays]
    net = WaveNetModel(
        batch_size=BATCH, dilations=PARAMS['dilations'], filter_width=2,
        residual_channels=32, dilation_channels=32, skip_channels=64,
        quantization_channels=256, use_biases=True, scalar_input=False,
        initial_filter_width=32, global_condition_channels=4,
        global_condition_cardinality=3)
    opt = optimizer_factory['adam'](learning_rate=train.LEARNING_RATE,
                                    momentum=train.MOMENTUM)
    mine = []
    for step in range(6):
        slots, T = R.plan(lengths, SIZE, 'pieces', train.CORPUS_SEED, step,
                          BATCH, ids)
        n = [s[2] for s in slots]
        loss = net.loss(R.gather(arrays, slots, T),
                        torch.tensor([s[3] for s in slots], dtype=torch.int32),
                        lengths=n)
        opt.minimize(loss)
        mine.append((str(step), '%.3f' % float(loss), str(sum(n))))
    assert mine == whole, (mine, whole)
    assert len(set(r for _, _, r in whole)) > 1      # (padded batches)


def test_a_run_continued_in_its_logdir_prints_the_next_steps(runs, tmp_path):
    import shutil
    log = str(tmp_path / 'b')
    shutil.copytree(runs['log_b'], log)
    rest = _losses(_run(runs['common'] + ['--num_steps', '6', '--logdir',
                                          log]))
    assert rest == runs['whole'][3:], (runs['whole'], rest)


def test_a_run_restored_into_a_new_logdir_takes_the_next_batches(runs,
                                                                 tmp_path):
    """--restore_from starts a new training at step 0, as it always did; the
    corpus goes on with the batch after the checkpoint's."""
    out = _run(runs['common'] + ['--num_steps', '3', '--restore_from',
                                 runs['log_b'], '--logdir_root',
                                 str(tmp_path / 'c')])
    assert 'Corpus batches continue at 3.' in out
    got = _losses(out)
    assert [k for k, _, _ in got] == ['0', '1', '2']
    assert [(v, r) for _, v, r in got] == \
        [(v, r) for _, v, r in runs['whole'][3:]], (runs['whole'], out)


UTTERANCE = ['--device_corpus', 'true', '--mask_padding', 'true',
             '--sample_size', str(SIZE), '--batch_size', str(BATCH),
             '--silence_threshold', '0.3', '--num_steps', '2',
             '--lc_features', 'mel', '--lc_channels', '8', '--lc_n_fft', '64',
             '--lc_feature_context', 'utterance', '--crop', 'random']


@pytest.mark.parametrize('model', [['--lc_upsample_scales', '4,4',
                                    '--lc_context', '2'], ['--lc_hop', '16']],
                         ids=['upsampler', 'rows'])
def test_train_utterance_context_features_run(hip_lib, wav_dir, tmp_path,
                                              model):
    params = str(tmp_path / 'params.json')
    json.dump(PARAMS, open(params, 'w'))
    got = _losses(_run(['--data_dir', wav_dir, '--wavenet_params', params,
                        '--logdir', str(tmp_path / 'run')] + UTTERANCE +
                       model))
    assert [s for s, _, _ in got] == ['0', '1']
    assert all(np.isfinite(float(v)) for _, v, _ in got)


def test_whole_utterance_frames_are_melspecs(hip_lib, wav_dir):
    """The corpus's frames of a whole-utterance item are MelSpec's of that
    utterance, bit for bit."""
    from wavenet import features
    from wavenet.corpus import DeviceCorpus, window_frames
    spec = features.MelSpec(16000, n_fft=64, hop=16, n_mels=8)
    _, arrays, _ = _reader_arrays(wav_dir)
    corpus = DeviceCorpus(wav_dir, 16000, False, silence_threshold=0.3,
                          spec=spec, seed=2)
    lengths = [a.shape[0] for a in arrays]
    assert corpus.frame_counts.tolist() == [-(-n // 16) for n in lengths]
    for step in range(3):
        (u, start, n, _), = R.plan(lengths, None, 'pieces', 2, step, 1)[0]
        assert start == 0 and n == lengths[u]
        b = corpus.batch(step, 1)
        want = spec(arrays[u]).cpu().numpy()
        F = want.shape[0]
        got = b.frames.cpu().numpy()
        assert got.shape == (1, window_frames(n, 16), 8)
        assert _same_bits(got[0, :F], want) and not _bits(got[0, F:]).any()
        assert b.offsets.tolist() == [0]
        rows = corpus.batch(step, 1, lc='rows').rows.cpu().numpy()
        assert _same_bits(rows[0], want[np.arange(n) // 16])
