"""Top-k / nucleus truncation of the draw, host side: the float64 restatement
(tests/trunc_ref.py) against a brute-force sort-based definition, the host
mask of wavenet/sampling.py against the restatement, argument validation of
the four generation entry points before the library or a device is touched,
generate.py's flags and its naive path."""
import os
import sys

import numpy as np
import pytest
import torch

import draw_ref as D
import trunc_ref as T
from util import ROOT

sys.path.insert(0, ROOT)

SETTINGS = [(1.0, 10, None), (0.7, None, 0.9), (3.0, 40, 0.8), (1.0, 1, None),
            (100.0, None, 0.5), (1.0, 3, 0.999)]


def _softmax32(logits):
    l = np.asarray(logits, np.float64)
    e = np.exp(l - l.max())
    return (e / e.sum()).astype(np.float32)


def _logits(kind, Q):
    # the vectors of tests/test_gpu_draw.py
    rng = np.random.default_rng(Q)
    if kind == 'random':
        return rng.normal(0, 4, Q).astype(np.float32)
    if kind == 'cliff':
        l = np.zeros(Q, np.float32)
        l[Q // 3] = 120.0
        l[[Q // 5, Q // 2 + 1, Q - 7]] = 110.0
        return l
    return (rng.integers(0, 3, Q) * 2.0 ** -20).astype(np.float32)


def _brute(p32, tau, K, P):
    """The kept set by sorting: codes in descending p; top-k takes the first
    K and every code equal to the K-th; the nucleus extends a prefix one
    whole tie group at a time until its mass reaches P * total."""
    p = np.asarray(p32, np.float32)
    Q = p.size
    order = sorted(range(Q), key=lambda q: -float(p[q]))
    if K is not None and K < Q:
        n = K
        while n < Q and p[order[n]] == p[order[K - 1]]:
            n += 1
        order = order[:n]
    w = D.weights(p, tau)
    if P is not None and float(np.float32(P)) != 1.0:
        total = sum(w[q] for q in order)
        bound = float(np.float32(P)) * total
        n, mass = 0, 0.0
        while n < len(order):
            m = n
            while m < len(order) and p[order[m]] == p[order[n]]:
                m += 1
            mass += float(np.sum(w[order[n:m]]))
            n = m
            if mass >= bound:
                break
        order = order[:n]
    keep = np.zeros(Q, bool)
    keep[order] = True
    return keep


@pytest.mark.parametrize('Q', [100, 256, 320, 512])
def test_restatement_matches_brute_force_and_host_mask(Q):
    from wavenet import sampling
    for kind in ('random', 'cliff', 'near_ties'):
        p = _softmax32(_logits(kind, Q))
        for tau, K, P in SETTINGS + [(1.0, Q, 1.0), (0.7, Q + 5, None),
                                     (1.0, None, 1e-6), (3.0, 2, 0.3)]:
            tau32 = float(np.float32(tau))
            w, keep, margin = T.truncate(p, tau32, K, P)
            what = (kind, Q, tau, K, P)
            if margin < 1e-9:
                continue
            assert np.array_equal(keep, _brute(p, tau32, K, P)), what
            assert np.array_equal(keep, sampling.kept_mask(p, tau, K, P)), what
            assert keep.any() and np.all(w[~keep] == 0), what
            assert np.array_equal(w[keep], D.weights(p, tau32)[keep]), what
            # kept codes are the most probable ones
            assert p[keep].min() >= (p[~keep].max() if (~keep).any() else 0), what
            if K is not None and K < Q:
                assert keep.sum() >= min(K, Q) or P is not None, what
            if K is None and P is None:
                assert keep.all()


def test_issue_settings_have_no_nucleus_tie():
    # the inputs of tests/test_gpu_trunc.py: margin well above 1e-9
    for Q in (100, 256, 320, 512):
        for kind in ('random', 'cliff', 'near_ties'):
            p = _softmax32(_logits(kind, Q))
            for tau, K, P in SETTINGS:
                m = T.truncate(p, float(np.float32(tau)), K, P)[2]
                assert m >= 1e-9, (Q, kind, tau, K, P, m)
    # top_k = 1 on the near-ties vector keeps the whole top tie group
    for Q, n in ((100, 36), (256, 83), (320, 112), (512, 181)):
        p = _softmax32(_logits('near_ties', Q))
        keep = T.truncate(p, 1.0, 1, None)[1]
        assert keep.sum() == n and np.array_equal(keep, p == p.max())


def test_host_mask_shapes_and_off():
    from wavenet import sampling
    rng = np.random.default_rng(0)
    p = np.stack([_softmax32(rng.normal(0, 3, 64)) for _ in range(6)]).reshape(2, 3, 64)
    assert sampling.kept_mask(p).all()
    assert sampling.kept_mask(p, 0.5, 64, 1.0).all()
    m = sampling.kept_mask(p, 0.8, 5, 0.9)
    assert m.shape == p.shape and m.dtype == bool
    for i in range(2):
        for j in range(3):
            assert np.array_equal(m[i, j], T.truncate(p[i, j], float(np.float32(0.8)), 5, 0.9)[1])
    assert sampling.resolve(None, None, 256) == (0, 0.0)
    assert sampling.resolve(256, 1.0, 256) == (0, 0.0)
    assert sampling.resolve(255, 0.5, 256) == (255, 0.5)


BAD = [dict(top_k=0), dict(top_k=-3), dict(top_k=True), dict(top_k=2.0),
       dict(top_k='4'), dict(top_p=0.0), dict(top_p=-0.1), dict(top_p=1.5),
       dict(top_p=float('nan')), dict(top_p=float('inf')), dict(top_p='x'),
       dict(top_p=True), dict(top_k=5, top_p=2.0)]


@pytest.mark.parametrize('bad', BAD, ids=[repr(sorted(b.items())) for b in BAD])
def test_bad_values_raise_before_library_or_device(bad, monkeypatch):
    from wavenet import WaveNetModel, _lib
    net = WaveNetModel(1, [1, 2, 4], 2, 32, 32, 32, quantization_channels=64,
                       device='cpu')
    monkeypatch.setattr(_lib, 'load', lambda: pytest.fail('library touched'))
    monkeypatch.setattr(_lib, 'require_gpu', lambda: pytest.fail('device touched'))
    calls = [lambda: net.generate(4, **bad),
             lambda: net.continue_generation(4, 3, **bad),
             lambda: net.generate_batch(4, [1, 2], **bad),
             lambda: net.continue_generation_batch(4, [3, 3], [1, 2], **bad)]
    for f in calls:
        with pytest.raises(ValueError, match='top_[kp]'):
            f()


def test_keywords_are_keyword_only_and_default_none():
    import inspect
    from wavenet import WaveNetModel
    for name in ('generate', 'continue_generation', 'generate_batch',
                 'continue_generation_batch'):
        ps = inspect.signature(getattr(WaveNetModel, name)).parameters
        for kw in ('top_k', 'top_p'):
            assert ps[kw].kind is inspect.Parameter.KEYWORD_ONLY, (name, kw)
            assert ps[kw].default is None, (name, kw)


def test_signatures_of_the_truncating_entries():
    from wavenet import _lib
    for name in ('wn_fastgen_run', 'wn_fastgen_run_wide', 'wn_fastgen_run_lc'):
        res, args = _lib.SIGNATURES[name]
        tres, targs = _lib.SIGNATURES[name + '_trunc']
        assert tres is res
        assert targs == args[:-1] + [_lib.c_int, _lib.c_float, _lib.P]
    with open(os.path.join(ROOT, 'include', 'wavenet_hip.h')) as f:
        header = f.read()
    for name in ('wn_fastgen_run_trunc', 'wn_fastgen_run_wide_trunc',
                 'wn_fastgen_run_lc_trunc'):
        assert 'int %s(' % name in header


def test_cli_parsing():
    import generate
    a = generate.get_arguments(['ckpt'])
    assert a.top_k is None and a.top_p is None
    a = generate.get_arguments(['ckpt', '--top_k', '40', '--top_p', '0.95'])
    assert a.top_k == 40 and a.top_p == 0.95
    assert generate.get_arguments(['ckpt', '--top_p', '1']).top_p == 1.0
    for bad in (['--top_k', '0'], ['--top_k', '-1'], ['--top_k', '2.5'],
                ['--top_k', 'x'], ['--top_p', '0'], ['--top_p', '1.01'],
                ['--top_p', 'nan'], ['--top_p', '-0.5']):
        with pytest.raises(SystemExit):
            generate.get_arguments(['ckpt'] + bad)


def test_naive_path_never_emits_a_dropped_code(tmp_path, monkeypatch):
    """generate.py --fast_generation false with a stubbed model whose
    predict_proba returns a known distribution: with --top_k 3 every code is
    one of the three most probable; with --top_p the nucleus."""
    import json
    import generate
    import wavenet
    Q = 32
    p = _softmax32(np.random.default_rng(5).normal(0, 2, Q))

    class Net(object):
        def __init__(self, **kw):
            pass

        def reserve(self, *a):
            pass

        def predict_proba(self, window, gc, local_condition=None):
            return torch.from_numpy(p)
    monkeypatch.setattr(wavenet, 'WaveNetModel', Net)
    monkeypatch.setattr(generate, 'restore', lambda *a, **k: None)
    params = dict(dilations=[1, 2], filter_width=2, residual_channels=32,
                  dilation_channels=32, quantization_channels=Q,
                  skip_channels=32, use_biases=True, scalar_input=False,
                  initial_filter_width=2, sample_rate=16000)
    pj = tmp_path / 'params.json'
    pj.write_text(json.dumps(params))
    for extra, (tau, K, P) in ((['--top_k', '3'], (1.0, 3, None)),
                               (['--top_p', '0.5', '--temperature', '0.7'],
                                (0.7, None, 0.5))):
        logdir = tmp_path / ('log' + extra[0])
        assert generate.main(['ckpt', '--fast_generation', 'false', '--samples',
                              '300', '--wavenet_params', str(pj), '--logdir',
                              str(logdir)] + extra) == 0
        out = [os.path.join(r, f) for r, _, fs in os.walk(str(logdir))
               for f in fs if f == 'generated_codes.npy']
        codes = np.load(out[0])[1:]
        keep = T.truncate(p, float(np.float32(tau)), K, P)[1]
        assert keep.sum() < Q and keep[codes].all()
        assert len(np.unique(codes)) > 1
