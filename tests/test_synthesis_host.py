"""The bulk synthesis path without a GPU: plan_rounds on written-out examples
and on seeded random lengths against tests/synth_ref.py, every ValueError of
synthesize and frame_distance before the library or a device is touched, the
new entry point's argument checks through the C ABI, and the two new
command-line errors."""
import os
import subprocess
import sys

import numpy as np
import pytest

import synth_ref as R
from util import ROOT

WN_ERR_BAD_SHAPE, WN_ERR_MISALIGNED, WN_ERR_NULL = -1, -3, -5


def _net(lc=None, **kw):
    from wavenet import WaveNetModel
    args = dict(batch_size=1, dilations=[1, 2, 4, 8], filter_width=2,
                residual_channels=32, dilation_channels=32, skip_channels=64,
                quantization_channels=256, use_biases=True, device='cpu')
    args.update(kw)
    return WaveNetModel(**args, local_condition_channels=lc)


# ---------------------------------------------------------------- plan_rounds
@pytest.mark.parametrize('lengths, batch, rounds, steps', [
    # ties: by index
    ([5, 9, 5, 9, 2], 2, [[1, 3], [0, 2], [4]], 9 + 5 + 2),
    # batch >= the number of items: one round
    ([3, 7, 1], 3, [[1, 0, 2]], 7),
    ([3, 7, 1], 256, [[1, 0, 2]], 7),
    # batch 1: one round per item, longest first
    ([3, 7, 1, 7], 1, [[1], [3], [0], [2]], 18),
    # a partial last round
    ([10, 20, 30, 40, 50], 3, [[4, 3, 2], [1, 0]], 70),
    ([1], 4, [[0]], 1),
])
def test_plan_rounds_examples(lengths, batch, rounds, steps):
    from wavenet import synthesis
    plan = synthesis.plan_rounds(lengths, batch)
    assert plan.rounds == rounds and plan.steps == steps
    assert plan.occupancy == sum(lengths) / float(batch * steps)
    assert R.plan_rounds(lengths, batch)[:2] == (rounds, steps)


@pytest.mark.parametrize('seed', range(6))
def test_plan_rounds_properties(seed):
    from wavenet import synthesis
    rng = np.random.default_rng(seed)
    U = int(rng.integers(1, 200))
    batch = int(rng.integers(1, 40))
    T = int(rng.integers(8, 20000))
    n = rng.integers(max(1, T // 8), T + 1, size=U)
    plan = synthesis.plan_rounds(n, batch)
    rounds, steps, occ = R.plan_rounds(n, batch)
    assert plan.rounds == rounds and plan.steps == steps
    assert sorted(u for r in plan.rounds for u in r) == list(range(U))
    flat = [int(n[u]) for r in plan.rounds for u in r]
    assert all(a >= b for a, b in zip(flat, flat[1:]))
    assert all(1 <= len(r) <= batch for r in plan.rounds)
    assert all(len(r) == batch for r in plan.rounds[:-1])
    # sorted rounds: a round's longest item is no longer than the mean of
    # the round before it
    assert plan.steps <= n.sum() / batch + n.max()
    assert plan.occupancy == n.sum() / float(batch * plan.steps) == occ
    assert 0 < plan.occupancy <= 1


@pytest.mark.parametrize('lengths, batch', [
    ([], 4), ([3, 0], 4), ([3, -1], 4), ([3.5], 4), ([[3]], 4), ([True], 4),
    ([3], 0), ([3], 257), ([3], 2.0), ([3], True)])
def test_plan_rounds_refuses(lengths, batch):
    from wavenet import synthesis
    with pytest.raises(ValueError):
        synthesis.plan_rounds(lengths, batch)


# ----------------------------------------------------------------- synthesize
@pytest.fixture
def untouchable(monkeypatch):
    """Builds the models, then makes the library and the device fail."""
    nets = dict(plain=_net(), rows=_net(lc=5),
                up=_net(lc=5, local_condition_upsample_scales=(2, 4)))
    from wavenet import _lib
    monkeypatch.setattr(_lib, 'load', lambda: pytest.fail('library touched'))
    monkeypatch.setattr(_lib, 'require_gpu',
                        lambda: pytest.fail('device touched'))
    return nets


def _rows(lengths, Lc=5):
    return [np.zeros((n, Lc), np.float32) for n in lengths]


@pytest.mark.parametrize('model, kw, what', [
    ('plain', dict(lengths=[], seeds=[]), 'at least one item'),
    ('plain', dict(lengths=[4, 0], seeds=[1, 2]), '>= 1'),
    ('plain', dict(lengths=[4, 3], seeds=[1]), '1 seeds for 2 items'),
    ('plain', dict(lengths=[4, 3], seeds=[1, 2, 3]), '3 seeds for 2 items'),
    ('rows', dict(lengths=[4, 3], seeds=[1, 2],
                  local_condition=_rows([4, 3], 6)), r'\[n, 5\]'),
    ('rows', dict(lengths=[4, 3], seeds=[1, 2],
                  local_condition=_rows([4, 2])), 'has 2 rows'),
    ('rows', dict(lengths=[4, 3], seeds=[1, 2],
                  local_condition=_rows([4])), 'list of 2'),
    # hop 8: 17 samples need 3 frames
    ('up', dict(lengths=[17, 8], seeds=[1, 2], frames=_rows([2, 1])),
     'has 2 rows'),
    ('up', dict(lengths=[17, 8], seeds=[1, 2], frames=_rows([3, 1]),
                local_condition=_rows([17, 8])), 'not both'),
    ('rows', dict(lengths=[4, 3], seeds=[1, 2], frames=_rows([4, 3]),
                  local_condition=_rows([4, 3])), 'not both'),
    ('rows', dict(lengths=[4, 3], seeds=[1, 2], frames=_rows([4, 3])),
     'frames are for models'),
    ('up', dict(lengths=[17, 8], seeds=[1, 2],
                local_condition=_rows([17, 8])), 'pass frames'),
    ('plain', dict(lengths=[4, 3], seeds=[1, 2],
                   local_condition=_rows([4, 3])), 'without local'),
    ('plain', dict(lengths=[4, 3], seeds=[1, 2], frames=_rows([4, 3])),
     'without local'),
    ('rows', dict(lengths=[4, 3], seeds=[1, 2]), 'is required'),
    ('up', dict(lengths=[17, 8], seeds=[1, 2]), 'are required'),
    ('plain', dict(lengths=[4], seeds=[1], batch=0), r'\[1, 256\]'),
    ('plain', dict(lengths=[4], seeds=[1], batch=257), r'\[1, 256\]'),
    ('plain', dict(lengths=[4], seeds=[1], first_samples=[256]), 'codes in'),
    ('plain', dict(lengths=[4, 3], seeds=[1, 2], first_samples=[3]),
     'codes in'),
    ('plain', dict(lengths=[4, 3], seeds=[1, 2],
                   global_condition=[1, 2, 3]), '3 ids for 2 items'),
    ('plain', dict(lengths=[4], seeds=[1], temperature=0.0), 'temperature'),
    ('plain', dict(lengths=[4], seeds=[1], top_k=0), 'top_k'),
    ('plain', dict(lengths=[4], seeds=[1], top_p=1.5), 'top_p'),
    # 2 streams x 1000 steps x 5 channels x 4 bytes = 40000 bytes
    ('rows', dict(lengths=[1000, 3], seeds=[1, 2], max_round_bytes=39999,
                  local_condition=_rows([1000, 3])),
     '40000 bytes.*39999.*smaller batch'),
])
def test_synthesize_refuses_before_any_device(untouchable, model, kw, what):
    from wavenet import synthesis
    kw = dict(kw)
    with pytest.raises(ValueError, match=what):
        synthesis.synthesize(untouchable[model], kw.pop('lengths'), **kw)


# ------------------------------------------------------------- frame_distance
@pytest.mark.parametrize('a, b, nframes, what', [
    ((2, 4, 8), (2, 4, 7), None, 'same shape'),
    ((2, 4, 8), (2, 5, 8), None, 'same shape'),
    ((4, 8), (1, 4, 8), None, 'same shape'),
    ((2, 4, 513), (2, 4, 513), None, '512'),
    ((8,), (8,), None, 'F, C'),
    ((2, 4, 8), (2, 4, 8), [1, 5], r'\[0, 4\]'),
    ((2, 4, 8), (2, 4, 8), [-1, 4], r'\[0, 4\]'),
    ((2, 4, 8), (2, 4, 8), [1], 'nframes must be 2'),
    ((2, 4, 8), (2, 4, 8), [1.0, 2.0], 'nframes must be 2'),
])
def test_frame_distance_refuses_before_any_device(untouchable, a, b, nframes,
                                                  what):
    from wavenet import features
    with pytest.raises(ValueError, match=what):
        features.frame_distance(np.zeros(a, np.float32),
                                np.zeros(b, np.float32), nframes)


def test_frame_distance_refuses_other_dtypes(untouchable):
    from wavenet import features
    x = np.zeros((2, 4, 8), np.float32)
    with pytest.raises(ValueError, match='float32'):
        features.frame_distance(x, x.astype(np.float64))


def test_summary_formula():
    import torch
    from wavenet import features
    d = features.FrameDistance(torch.tensor([8.0, 4.0], dtype=torch.float64),
                               torch.tensor([1.0, 1.0], dtype=torch.float64),
                               torch.tensor([3.0, 1.5], dtype=torch.float64))
    mae, lsd = d.summary([2, 1], 4)
    k = 10.0 / np.log(10.0)
    assert mae == k * 12.0 / (3 * 4) and lsd == k * 4.5 / 3
    with pytest.raises(ValueError):
        d.summary([0, 0], 4)
    with pytest.raises(ValueError):
        d.summary([1], 4)


def test_distance_entry_checks_arguments_without_a_device(hip_lib):
    """wn_feature_distance's checks come before any launch: bad arguments
    give their codes on a machine without a GPU (the addresses are never
    read)."""
    f = hip_lib.wn_feature_distance
    p, d = 1 << 20, 1 << 21
    assert hip_lib.wn_feature_distance_partials(1, 1) == 3
    assert hip_lib.wn_feature_distance_partials(3, 64) == 9
    assert hip_lib.wn_feature_distance_partials(3, 65) == 18
    for B, F in ((0, 1), (1, 0), (-1, 4), (65536, 32768)):
        assert hip_lib.wn_feature_distance_partials(B, F) == -1
    for args in ((None, p), (p, None)):
        assert f(*args, 1, 4, 4, None, d, d, d, d, None) == WN_ERR_NULL
    for k in range(4):
        outs = [d] * 4
        outs[k] = None
        assert f(p, p, 1, 4, 4, None, *outs, None) == WN_ERR_NULL
    for B, F, C in ((1, 1, 0), (1, 1, 513), (0, 1, 4), (1, 0, 4), (-1, 4, 4),
                    (65536, 32768, 4)):
        assert f(p, p, B, F, C, None, d, d, d, d, None) == WN_ERR_BAD_SHAPE
    for args in ((p + 4, p, 1, 4, 4, None, d, d, d, d),
                 (p, p + 8, 1, 4, 4, None, d, d, d, d),
                 (p + 2, p, 1, 4, 3, None, d, d, d, d),
                 (p, p, 1, 4, 4, p + 2, d, d, d, d),
                 (p, p, 1, 4, 4, None, d + 4, d, d, d),
                 (p, p, 1, 4, 4, None, d, d + 4, d, d),
                 (p, p, 1, 4, 4, None, d, d, d + 4, d),
                 (p, p, 1, 4, 4, None, d, d, d, d + 4)):
        assert f(*args, None) == WN_ERR_MISALIGNED


# --------------------------------------------------------------- command line
def _error_of(script, argv):
    p = subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv,
                       cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    return p.returncode, p.stderr.decode()


@pytest.mark.parametrize('other', [['--lc_wav', 'a.wav'],
                                   ['--lc_path', 'a.npy']])
def test_generate_lc_wav_dir_excludes_single_inputs(other):
    code, err = _error_of('generate.py', ['ckpt', '--lc_wav_dir', 'in',
                                          '--wav_out_dir', 'out'] + other)
    assert code == 2 and 'give either --lc_wav_dir or %s' % other[0] in err


def test_evaluate_synthesis_flags_need_synthesis():
    code, err = _error_of('evaluate.py', ['ckpt', '--data_dir', 'in',
                                          '--synthesis_out', 'out'])
    assert code == 2 and '--synthesis_out needs --synthesis true' in err
