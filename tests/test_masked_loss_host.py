"""The masked loss (`lengths` on WaveNetModel.loss / loss_from_codes) without
a GPU: the argument checks before any library or device is touched, the
reader's dequeue_lengths, wn_xent_masked's argument validation, the float64
masked reference (tests/masked_ref.py) against the existing reference run on
every clip alone, and the data-parallel denominator on two gloo ranks."""
import ctypes
import inspect
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
from scipy.io import wavfile

import lc_ref
import masked_ref
import masked_dp_worker
from util import ROOT

sys.path.insert(0, ROOT)


def _net(**kw):
    from wavenet import WaveNetModel
    args = dict(batch_size=3, dilations=[1, 2, 4, 8], filter_width=2,
                residual_channels=32, dilation_channels=32, skip_channels=64,
                quantization_channels=256, use_biases=True, device='cpu')
    args.update(kw)
    return WaveNetModel(**args)


# ---- arguments ---------------------------------------------------------------
def test_keyword_only_and_default_none():
    from wavenet import WaveNetModel
    for fn in (WaveNetModel.loss, WaveNetModel.loss_from_codes):
        for name in ('lengths', 'loss_denominator'):
            p = inspect.signature(fn).parameters[name]
            assert p.kind == p.KEYWORD_ONLY and p.default is None, (fn, name)


T = 10
BAD = [
    (dict(lengths=[10, 5]), 'shape'),                       # B = 3
    (dict(lengths=[[10, 5, 3]]), 'shape'),
    (dict(lengths=7), 'shape'),
    (dict(lengths=[10.0, 5.0, 3.0]), 'integers'),
    (dict(lengths=np.array([10, 5, 3], np.float32)), 'integers'),
    (dict(lengths=torch.tensor([10., 5., 3.])), 'integers'),
    (dict(lengths=[True, True, False]), 'integers'),
    (dict(lengths=np.array([1, 1, 1], bool)), 'integers'),
    (dict(lengths=['a', 'b', 'c']), 'integers'),
    (dict(lengths=[10, 0, 3]), r'\[1, 10\]'),
    (dict(lengths=[10, -2, 3]), r'\[1, 10\]'),
    (dict(lengths=[11, 5, 3]), r'\[1, 10\]'),
    (dict(lengths=torch.tensor([10, 5, 30])), r'\[1, 10\]'),
    (dict(loss_denominator=18.0), 'needs lengths'),
    (dict(lengths=[10, 5, 3], loss_denominator=0), 'positive finite'),
    (dict(lengths=[10, 5, 3], loss_denominator=-4.0), 'positive finite'),
    (dict(lengths=[10, 5, 3], loss_denominator=float('nan')),
     'positive finite'),
    (dict(lengths=[10, 5, 3], loss_denominator=float('inf')),
     'positive finite'),
    (dict(lengths=[10, 5, 3], loss_denominator='18'), 'positive finite'),
    (dict(lengths=[10, 5, 3], loss_denominator=True), 'positive finite'),
]


@pytest.mark.parametrize('kw, what', BAD, ids=[str(i) for i in range(len(BAD))])
def test_bad_arguments_raise_before_library_or_device(kw, what, monkeypatch):
    from wavenet import _lib
    net = _net()
    net._check_supported = lambda: None    # (a CPU model: stop before launches)
    monkeypatch.setattr(_lib, 'load', lambda: pytest.fail('library touched'))
    monkeypatch.setattr(_lib, 'require_gpu',
                        lambda: pytest.fail('device touched'))
    with pytest.raises(ValueError, match=what):
        net.loss(np.zeros((3, T), np.float32), **kw)
    with pytest.raises(ValueError, match=what):
        net.loss_from_codes(torch.zeros((3, T), dtype=torch.int32), **kw)


def test_check_lengths_accepts():
    from wavenet.model import check_lengths
    assert check_lengths(None, None, 3, T, 'loss') is None
    for ok in ([10, 1, 2], np.array([10, 1, 2], np.int64),
               np.array([10, 1, 2], np.uint8), torch.tensor([10, 1, 2]),
               torch.tensor([10, 1, 2], dtype=torch.int32)):
        n, den = check_lengths(ok, None, 3, T, 'loss')
        assert n.dtype == np.int32 and n.tolist() == [10, 1, 2] and den == 13.0
    assert check_lengths([10, 1, 2], 6.5, 3, T, 'loss')[1] == 6.5
    assert check_lengths([10, 1, 2], np.float32(8), 3, T, 'loss')[1] == 8.0
    assert check_lengths([10, 1, 2], 26, 3, T, 'loss')[1] == 26.0


# ---- entry point -----------------------------------------------------------------
def test_wn_xent_masked_validates_arguments(hip_lib):
    lib = hip_lib
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    p16 = p + (-p) % 16
    call = lambda logits=p16, ld=256, q=p16, n=p16, inv=p16, dl=p16, \
        parts=p16, B=2, T=3, Q=256: lib.wn_xent_masked(
            logits, ld, q, n, inv, dl, parts, B, T, Q, 1, None)
    for name in ('logits', 'q', 'n', 'inv', 'parts'):
        assert call(**{name: None}) == -5, name          # WN_ERR_NULL
    for name in ('B', 'T', 'Q'):
        assert call(**{name: 0}) == -1, name             # WN_ERR_BAD_SHAPE
        assert call(**{name: -4}) == -1, name
    assert call(Q=254) == -2 and call(ld=258) == -2      # WN_ERR_UNSUPPORTED
    assert call(logits=p16 + 4) == -3                    # WN_ERR_MISALIGNED
    assert call(dl=p16 + 8) == -3
    assert call(n=p16 + 2) == -3 and call(inv=p16 + 1) == -3
    # the unmasked entry point is unchanged
    assert lib.wn_xent(None, 256, p16, p16, p16, 2, 3, 256, 1, None) == -5
    assert lib.wn_xent_partials(8 * 16000) == 1024


# ---- reader ------------------------------------------------------------------
def _corpus(d, sizes, Lc=None, hop=None):
    rng = np.random.default_rng(0)
    for i, n in enumerate(sizes):
        a = rng.uniform(-0.9, 0.9, n)
        wavfile.write(os.path.join(d, 'c%02d.wav' % i), 16000,
                      (a * 32767).astype(np.int16))
        if Lc:
            np.save(os.path.join(d, 'c%02d.npy' % i), rng.standard_normal(
                ((n + hop - 1) // hop, Lc)).astype(np.float32))


def _drain(reader, batch, steps):
    out = []
    reader.start_threads()
    try:
        for _ in range(steps):
            a = reader.dequeue(batch)
            out.append((a, reader.dequeue_lengths(batch)))
            if reader.lc_enabled:
                lc = reader.dequeue_lc_frames(batch) if reader.lc_frames \
                    else reader.dequeue_lc(batch)
                out[-1] += (lc,)
        with pytest.raises(ValueError, match='must follow'):
            reader.dequeue_lengths(batch)
    finally:
        reader.coord.request_stop()
        reader.coord.join(reader.threads)
    return out


SIZES = [700, 1300, 1000]


@pytest.mark.parametrize('sample_size', [None, 600])
@pytest.mark.parametrize('lc', [None, 'rows', 'frames'])
def test_dequeue_lengths(tmp_path, sample_size, lc):
    from wavenet import AudioReader
    hop, Lc = 20, 3
    _corpus(str(tmp_path), SIZES, Lc if lc else None, hop)
    reader = AudioReader(str(tmp_path), None, sample_rate=16000,
                         gc_enabled=False, sample_size=sample_size,
                         silence_threshold=None, seed=0,
                         lc_channels=Lc if lc else None,
                         lc_hop=hop if lc else None, lc_frames=lc == 'frames')
    want = [p.shape[0] for p, _, _ in reader.iter_pieces()]
    if sample_size is None:
        assert sorted(want) == sorted(SIZES)
    else:
        assert max(want) == 600 and min(want) < 600
        assert sum(want) == sum(SIZES)
    reader._rng.seed(0)           # (the same file order again for the queue)
    batch = 3
    seen = []
    for item in _drain(reader, batch, 2):
        a, n = item[0], item[1]
        assert n.dtype == torch.int64 and tuple(n.shape) == (batch,)
        assert a.shape[1] == int(n.max())
        for b in range(batch):
            k = int(n[b])
            assert 1 <= k <= a.shape[1]
            # real samples up to the length (the corpus has no exact zeros),
            # zero padding behind it
            assert float(a[b, :k].abs().min()) > 0
            assert float(a[b, k:].abs().sum()) == 0
            if lc == 'rows':
                assert tuple(item[2].shape) == (batch, a.shape[1], Lc)
                assert float(item[2][b, :k].abs().min()) > 0
                assert float(item[2][b, k:].abs().sum()) == 0
            if lc == 'frames':
                fr, off = item[2]
                assert fr.shape[0] == batch and off.shape[0] == batch
                assert fr.shape[1] * hop >= int(off[b]) + k
        seen += n.tolist()
    # the queue order is the pieces' order (the first pass, then the next)
    assert seen[:len(want)] == want[:len(seen)]


# ---- the float64 reference -----------------------------------------------------
def _tree_err(a, b):
    fa, fb = dict(lc_ref.flatten(a)), dict(lc_ref.flatten(b))
    assert sorted(fa) == sorted(fb)
    return max(np.abs(fa[k] - fb[k]).max() / max(np.abs(fb[k]).max(), 1e-300)
               for k in fa)


REF_CASES = [
    # (Q, biases, gc, Lc, lengths, T)
    (16, True, None, None, [23, 9, 1, 2], 23),
    (16, False, 3, None, [5, 23], 23),
    (32, True, 2, 4, [40, 17, 2], 40),
    (16, True, None, 3, [1, 30, 30], 30),
]


@pytest.mark.parametrize('case', REF_CASES,
                         ids=['plain', 'gc_nob', 'gc_lc', 'lc'])
def test_masked_reference_is_the_clips_alone(case):
    """loss_and_grads on the padded batch == sum_b lengths[b] * (L_b, g_b) / D
    of lc_ref on every clip alone and unpadded, to float64 round-off; the
    padding's content (codes and LC rows) does not enter."""
    from wavenet import WaveNetModel
    Q, biases, gc, Lc, lengths, T = case
    B, dil = len(lengths), [1, 2, 4, 8, 1, 2]
    kw = {}
    if gc:
        kw.update(global_condition_channels=gc, global_condition_cardinality=gc)
    net = WaveNetModel(B, dil, 2, 8, 8, 16, quantization_channels=Q,
                       use_biases=biases, device='cpu', seed=B,
                       local_condition_channels=Lc, **kw)
    with torch.no_grad():
        g = torch.Generator().manual_seed(1)
        for n, v in net.named_variables():
            if 'bias' in n.split('/')[-1]:
                v.copy_(0.1 * torch.randn(v.shape, generator=g))
    var = lc_ref.model_tree(net)
    rng = np.random.default_rng(T)
    codes = rng.integers(0, Q, (B, T))
    lc = rng.standard_normal((B, T, Lc)) if Lc else None
    ids = None if gc is None else np.arange(B) % gc
    args = dict(gc_ids=ids, use_biases=biases, quantization_channels=Q)
    loss, grads = masked_ref.loss_and_grads(var, dil, codes, lengths, lc,
                                            **args)
    want_loss, want = masked_ref.clipwise(var, dil, codes, lengths, lc, **args)
    assert abs(loss - want_loss) <= 1e-13 * max(1.0, abs(want_loss))
    assert _tree_err(grads, want) <= 1e-11
    assert max(np.abs(a).max() for _, a in lc_ref.flatten(want)) > 0
    # other padding, same numbers
    codes2, lc2 = codes.copy(), None if lc is None else lc.copy()
    for b, n in enumerate(lengths):
        codes2[b, n:] = rng.integers(0, Q, T - n)
        if lc is not None:
            lc2[b, n:] = rng.standard_normal((T - n, Lc))
    loss2, grads2 = masked_ref.loss_and_grads(var, dil, codes2, lengths, lc2,
                                              **args)
    assert abs(loss2 - loss) <= 1e-13 * max(1.0, abs(loss))
    assert _tree_err(grads2, grads) <= 1e-11
    # full lengths: the unmasked reference
    full = [T] * B
    la, ga = masked_ref.loss_and_grads(var, dil, codes, full, lc, **args)
    lb, gb = lc_ref.loss_and_grads(var, dil, codes, lc, **args)
    assert abs(la - lb) <= 1e-13 * max(1.0, abs(lb))
    assert _tree_err(ga, gb) <= 1e-11
    # a denominator of the caller's: a plain rescaling
    ld, gd = masked_ref.loss_and_grads(var, dil, codes, lengths, lc,
                                       denominator=2.5 * sum(lengths), **args)
    assert abs(ld * 2.5 - loss) <= 1e-13 * max(1.0, abs(loss))
    assert _tree_err(_scaled(gd, 2.5), grads) <= 1e-11


def _scaled(tree, k):
    if isinstance(tree, dict):
        return {n: _scaled(v, k) for n, v in tree.items()}
    if isinstance(tree, list):
        return [_scaled(v, k) for v in tree]
    return k * tree


# ---- data-parallel ---------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_masked_denominator_single_process():
    from wavenet import parallel
    assert parallel.masked_denominator([5, 7, 1]) == 13.0
    assert parallel.masked_denominator(np.array([16000, 9000])) == 25000.0
    assert parallel.masked_denominator(torch.tensor([3, 4])) == 7.0


def test_two_ranks_share_the_denominator(tmp_path):
    """Two gloo ranks with different lengths get the same D = (global sum) /
    world, and their averaged float64 gradients (and mean loss) are the
    single-process masked reference on the concatenated batch."""
    world = 2
    mp.spawn(masked_dp_worker.worker,
             args=(world, _free_port(), str(tmp_path)), nprocs=world,
             join=True)
    dil, Q, codes, lengths = masked_dp_worker.batch(world)
    assert lengths[:2].sum() != lengths[2:].sum()
    loss, g = masked_ref.loss_and_grads(
        masked_dp_worker.variables(Q), dil, codes, lengths, use_biases=True,
        quantization_channels=Q)
    full = np.concatenate([a.reshape(-1) for _, a in lc_ref.flatten(g)])
    assert np.abs(full).max() > 0
    for r in range(world):
        got = np.load(os.path.join(str(tmp_path), 'rank%d.npz' % r))
        assert float(got['den']) == lengths.sum() / float(world)
        assert np.abs(got['grads'] - full).max() <= 1e-13 * np.abs(full).max()
        assert abs(float(got['loss']) - loss) <= 1e-13 * max(1.0, abs(loss))
