"""Mixture-of-logistics head, host side (no device): the rule defines a
distribution over the 65536 levels, its cancellation-free form is the naive
one, wavenet/mol.py's float32 statement follows tests/mol_ref.py's float64
one, the level and sampling rules, the sampling fixtures lie off every
rounding boundary, the constructor's and the command line's refusals, the
checkpoint entry, and the binding table against include/wavenet_mol.h."""
import glob
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import mol_cases as MC
import mol_ref as R
from util import ROOT, TINY, cfg_with, model_kwargs

HEADER = 'wavenet_mol.h'


def _lp_all_levels(mu, beta, form):
    j = torch.arange(R.C)
    with torch.no_grad():
        return R.log_bin(j, torch.tensor(mu, dtype=torch.float64),
                         torch.tensor(beta, dtype=torch.float64), form).numpy()


@pytest.mark.parametrize('beta', [-14, -11, -6, 0, 1])
@pytest.mark.parametrize('mu', [-1.2, -1, 0, 0.3, 1])
def test_the_bins_sum_to_one(mu, beta):
    lp = _lp_all_levels(float(mu), float(beta), 'stable')
    assert abs(math.fsum(np.exp(lp)) - 1.0) < 1e-12
    # the package's statement of the rule, in float64, is the same function
    from wavenet import mol
    j = np.arange(R.C)
    lg = np.zeros((R.C, 12))
    lg[:, 4], lg[:, 8] = mu, beta
    nll, _ = mol.loss_reference(lg, j, 1, -14.0, 1.0, dtype=np.float64)
    assert abs(math.fsum(np.exp(-nll)) - 1.0) < 1e-12
    assert np.abs(-nll - lp).max() <= 1e-12 * np.maximum(1, np.abs(lp)).max()


@pytest.mark.parametrize('beta', [-14, -11, -6, 0, 1])
@pytest.mark.parametrize('mu', [-1.2, -1, 0, 0.3, 1])
def test_naive_and_stable_forms_agree(mu, beta):
    naive = _lp_all_levels(float(mu), float(beta), 'naive')
    stable = _lp_all_levels(float(mu), float(beta), 'stable')
    well = np.exp(stable) > 1e-3
    if beta <= -11:
        assert well.any()
    assert np.abs(naive - stable)[well].max(initial=0.0) < 1e-9


@pytest.mark.parametrize('K', [1, 4, 10, 32])
def test_float32_statement_follows_float64(K):
    """mol.loss_reference in float64 equals mol_ref's autograd gradients: the
    hand-written derivatives are the derivatives."""
    from wavenet import mol
    lg, lv = MC.kernel_case(3, 37, K)
    tgt = R.targets(lv).reshape(-1)
    inv = 1.0 / len(tgt)
    n64, g64 = R.loss_rows(lg[:, :3 * MC.padded(K)], tgt, K, MC.LSM, inv)
    nm, gm = mol.loss_reference(lg, tgt, K, MC.LSM, inv, dtype=np.float64)
    assert np.isfinite(nm).all() and np.isfinite(gm).all()
    assert np.abs(nm - n64).max() <= 1e-9 * np.maximum(1, np.abs(n64)).max()
    Kp = MC.padded(K)
    for blk in range(3):
        a = gm[:, blk * Kp:blk * Kp + K]
        b = np.nan_to_num(g64[:, blk * Kp:blk * Kp + K])
        assert np.abs(a - b).max() <= 1e-9 * max(1.0, np.abs(b).max()), blk
        assert (gm[:, blk * Kp + K:(blk + 1) * Kp] == 0).all()
    assert (gm[tgt < 0] == 0).all() and (nm[tgt < 0] == 0).all()


def test_levels_reference():
    from wavenet import mol
    y = np.array([-1.0, 1.0, -1.5, 7.0, 0.0, np.nan], np.float32)
    lv, c = mol.levels_reference(y)
    assert lv.tolist() == [0, 65535, 0, 65535, 32768, 0]   # (32767.5: to even)
    assert c[0] == -1.0 and c[1] == 1.0 and c.dtype == np.float32
    # +-0.5 / 65535 around the boundary between levels j and j + 1
    for j in (0, 1, 1000, 40000, 65534):
        edge = (2 * j + 1) / 65535.0 - 1.0
        lo = np.float32(edge - 0.5 / 65535)
        hi = np.float32(edge + 0.5 / 65535)
        got, _ = mol.levels_reference(np.array([lo, hi], np.float32))
        assert got.tolist() == [j, j + 1]
    # the grid is a fixed point, symmetric, and equals the float64 rule
    j = np.arange(65536)
    cj = mol.centres(j)
    assert np.array_equal(mol.levels_reference(cj)[0], j)
    assert np.array_equal(cj, -cj[::-1])
    assert np.abs(cj - R.centres(j)).max() < 2.0 ** -24
    y = np.random.default_rng(0).uniform(-1.1, 1.1, 4096).astype(np.float32)
    frac = (np.clip(y.astype(np.float64), -1, 1) + 1) * 32767.5
    away = np.abs(frac - np.floor(frac) - 0.5) > 0.01
    assert np.array_equal(mol.levels_reference(y)[0][away], R.levels(y)[away])
    # lengths: level 0 and centre exactly 0 at and behind them
    lv, c = mol.levels_reference(np.full((2, 5), 0.5, np.float32), [3, 0])
    assert lv[0].tolist()[3:] == [0, 0] and (c[0, 3:] == 0).all()
    assert not lv[1].any() and not c[1].any() and lv[0, 0] == 49151


@pytest.mark.parametrize('K', MC.SAMPLE_K)
def test_sample_reference_and_its_fixtures(K):
    """A pure function of (seed, counter); and no fixture draw lies within
    1e-9 levels of a rounding boundary, so the device comparison of levels is
    exact with nothing left out."""
    from wavenet import mol
    p, seeds, counters = MC.sample_fixture(K)
    for tau in MC.SAMPLE_TEMPERATURES:
        lv, ce, x = mol.sample_reference(p, seeds, counters, tau,
                                         return_x=True)
        perm = np.random.default_rng(1).permutation(len(p))
        lv2, ce2 = mol.sample_reference(p[perm], seeds[perm], counters[perm],
                                        tau)
        assert np.array_equal(lv[perm], lv2) and np.array_equal(ce[perm], ce2)
        one = mol.sample_reference(p[3:4], seeds[3:4], counters[3:4], tau)
        assert one[0][0] == lv[3]
        frac = (np.clip(x, -1, 1) + 1) * 32767.5
        dist = np.abs(frac - np.floor(frac) - 0.5)
        inside = np.abs(x) < 1
        assert (dist[inside] > 1e-9).all()
        assert np.array_equal(ce, mol.centres(lv))
        assert 0 <= lv.min() and lv.max() <= 65535
        if tau == 0.0:
            # the mean of the picked component, snapped
            assert set(np.unique(lv)) <= set(np.unique(
                R.levels(p[:, 1].astype(np.float64))))
    # u2 with all bits 0: log(0) = -inf, the clamp gives level 0; u1 = 0 picks
    # the first component of weight > 0
    u = np.zeros((len(p), 2))
    lv, _ = mol.sample_reference(p, seeds, counters, 1.0, uniforms=u)
    assert not lv.any()
    lv, _ = mol.sample_reference(p, seeds, counters, 0.0, uniforms=u)
    assert np.array_equal(lv, R.levels(p[:, 1, 0].astype(np.float64)))
    # the uniform is csrc/wn_common.h's
    import draw_ref
    for s, c in ((0, 0), (12345, 7), (-5, 2 ** 40)):
        assert mol.draw_uniform(s, c) == draw_ref.uniform(s, c)


# ------------------------------------------------------------ constructor
def _net(**kw):
    from wavenet import WaveNetModel
    cfg = cfg_with(TINY, batch_size=1, scalar_input=True,
                   initial_filter_width=4)
    args = model_kwargs(cfg)
    args.update(kw)
    return WaveNetModel(device='cpu', **args)


def test_constructor_keywords(hip_lib):
    from wavenet import WaveNetModel
    sig = inspect.signature(WaveNetModel.__init__).parameters
    for name, default in (('output_mixture', None),
                          ('mixture_log_scale_min', -14.0)):
        assert sig[name].kind == sig[name].KEYWORD_ONLY
        assert sig[name].default == default
    plain, net = _net(), _net(output_mixture=10)
    assert plain.Q == 16 and plain.mol_K == 0
    assert net.Q == 36 and net.mol_K == 10 and net.mol_Kp == 12
    assert net.variables['postprocessing']['postprocess2'].shape == (1, 16, 36)
    assert _net(output_mixture=1).Q == 12 and _net(output_mixture=32).Q == 96
    # quantization_channels is not read by the network
    assert _net(output_mixture=4, quantization_channels=7).Q == 12
    # local conditioning goes with scalar_input under a mixture head; a
    # scalar-input softmax model stays refused
    with pytest.raises(NotImplementedError, match='scalar_input without'):
        _net(local_condition_channels=5)
    assert _net(output_mixture=4, local_condition_channels=5).Lc == 5
    assert _net(output_mixture=4, local_condition_channels=5,
                local_condition_upsample_scales=(2, 4),
                local_condition_context=1).lc_hop == 8


@pytest.mark.parametrize('kw,what', [
    (dict(output_mixture=0), 'output_mixture'),
    (dict(output_mixture=33), 'output_mixture'),
    (dict(output_mixture=2.0), 'output_mixture'),
    (dict(output_mixture=True), 'output_mixture'),
    (dict(output_mixture=4, scalar_input=False), 'scalar_input'),
    (dict(output_mixture=4, mixture_log_scale_min=-0.5), 'log_scale_min'),
    (dict(output_mixture=4, mixture_log_scale_min=-33), 'log_scale_min'),
    (dict(output_mixture=4, mixture_log_scale_min=None), 'log_scale_min'),
])
def test_constructor_refusals_touch_nothing(kw, what, monkeypatch):
    from wavenet import _lib
    monkeypatch.setattr(_lib, 'load', lambda: pytest.fail('library touched'))
    monkeypatch.setattr(_lib, 'require_gpu',
                        lambda: pytest.fail('device touched'))
    with pytest.raises(ValueError, match=what):
        _net(**kw)


def test_entry_points_that_take_codes_refuse(hip_lib):
    from wavenet.input_noise import InputNoise
    net = _net(output_mixture=4)
    q = torch.zeros((1, 8), dtype=torch.int32)
    for call in (lambda: net.loss_from_codes(q),
                 lambda: net.score_from_codes(q),
                 lambda: net.loss_from_codes(q, input_codes=q)):
        with pytest.raises(ValueError, match='no mu-law codes'):
            call()
    with pytest.raises(ValueError, match='predict_mixture'):
        net.predict_proba([1, 2, 3])
    with pytest.raises(ValueError, match='predict_proba'):
        _net().predict_mixture([0.1, 0.2])
    noise = InputNoise(0.1, 2)
    for fn in (net.loss, net.score):
        with pytest.raises(ValueError, match='not for a mixture'):
            fn(np.zeros((1, 8), np.float32), input_noise=noise,
               noise_keys=[1])
    # fast and batched generation: refused, and named as the follow-up
    for call in (lambda: net.generate(4), lambda: net.generate_batch(4, [1]),
                 lambda: net.predict_proba_incremental(3),
                 lambda: _net().generate(4)):
        with pytest.raises(NotImplementedError, match='follow-up'):
            call()


def test_train_flag_errors_name_both(tmp_path, capsys):
    import json
    import train
    params = dict(filter_width=2, sample_rate=16000, dilations=[1, 2],
                  residual_channels=32, dilation_channels=32,
                  quantization_channels=64, skip_channels=32, use_biases=True,
                  scalar_input=False, initial_filter_width=4)
    onehot, scalar = str(tmp_path / 'a.json'), str(tmp_path / 'b.json')
    json.dump(params, open(onehot, 'w'))
    json.dump(dict(params, scalar_input=True), open(scalar, 'w'))
    for argv, words in (
            (['--wavenet_params', onehot, '--output_mixture', '4'],
             ('--output_mixture', 'scalar_input')),
            (['--wavenet_params', scalar, '--mixture_log_scale_min', '-9'],
             ('--mixture_log_scale_min', '--output_mixture')),
            (['--wavenet_params', scalar, '--output_mixture', '0'],
             ('--output_mixture', 'from 1 to 32')),
            (['--wavenet_params', scalar, '--output_mixture', '4',
              '--mixture_log_scale_min', '-0.5'],
             ('--mixture_log_scale_min', 'from -32 to -1'))):
        with pytest.raises(SystemExit) as e:
            train.get_arguments(['--synthetic'] + argv)
        err = capsys.readouterr().err
        assert e.value.code == 2 and all(w in err for w in words), err
    a = train.get_arguments(['--synthetic', '--wavenet_params', scalar,
                             '--output_mixture', '10'])
    assert a.mixture == (10, -14.0)
    a = train.get_arguments(['--synthetic', '--wavenet_params', scalar])
    assert a.mixture is None


def test_checkpoint_entry_round_trip(tmp_path):
    from wavenet import mol
    e = mol.output_entry(10, -14.0)
    assert e == {'kind': 'mol', 'components': 10, 'log_scale_min': -14.0,
                 'levels': 65536}
    path = str(tmp_path / 'ck.pt')
    torch.save({'output': e}, path)
    back = torch.load(path)['output']
    assert back == e and mol.check_entry(back) == (10, -14.0)
    assert mol.check_entry(None) is None
    for bad in ({'kind': 'softmax'}, dict(e, levels=256),
                dict(e, components=40), dict(e, log_scale_min=0.0), 'mol'):
        with pytest.raises(ValueError):
            mol.check_entry(bad)
    mol.same_entry(e, 10, -14.0)
    mol.same_entry(None, None, -14.0)
    for stored, K, lsm in ((e, 4, -14.0), (e, 10, -12.0), (e, None, -14.0),
                           (None, 10, -14.0)):
        with pytest.raises(ValueError) as err:
            mol.same_entry(stored, K, lsm)
        assert 'checkpoint' in str(err.value) and 'this run' in str(err.value)


# ----------------------------------------------------------------- bindings
def _declarations(header):
    src = open(os.path.join(ROOT, 'include', header)).read()
    src = re.sub(r'/\*.*?\*/', ' ', src, flags=re.S)
    return {m.group(2): (m.group(1), [' '.join(p.split())
                                      for p in m.group(3).split(',')])
            for m in re.finditer(
                r'\b(int|long)\s+(wn_\w+)\s*\(([^)]*)\)\s*;', src)}


def test_binding_table_matches_its_header():
    from wavenet import _lib
    decl = _declarations(HEADER)
    assert set(decl) == {'wn_mol_quantize', 'wn_mol_loss', 'wn_mol_score',
                         'wn_mol_score_scratch_floats', 'wn_mol_params_row',
                         'wn_mol_sample'}
    assert set(_lib.MOL_SIGNATURES) == set(decl)
    ctype = {'int': _lib.c_int, 'long': _lib.c_long, 'float': _lib.c_float,
             'double': _lib.c_double}
    for name, (res, params) in decl.items():
        want = [_lib.P if '*' in p else ctype[p.split()[0]] for p in params]
        assert _lib.MOL_SIGNATURES[name] == (ctype[res], want), name
    for path in glob.glob(os.path.join(ROOT, 'include', '*.h')):
        other = os.path.basename(path)
        if other != HEADER:
            assert not set(decl) & set(_declarations(other)), other
    for name, table in vars(_lib).items():
        if name.endswith('SIGNATURES') and name != 'MOL_SIGNATURES':
            assert not set(decl) & set(table), name


def test_load_binds_the_table(hip_lib):
    from wavenet import _lib
    for name, (res, args) in _lib.MOL_SIGNATURES.items():
        fn = getattr(hip_lib, name)
        assert fn.restype is res and fn.argtypes == args, name


def test_every_writing_entry_of_the_header_is_guarded():
    import test_gpu_guard_mol as tg
    w = {k: [p for p in v[1] if '*' in p and not p.startswith('const ')
             and not re.search(r'\bstream$', p)]
         for k, v in _declarations(HEADER).items()}
    w = {k: v for k, v in w.items() if v}
    assert set(w) == {'wn_mol_quantize', 'wn_mol_loss', 'wn_mol_score',
                      'wn_mol_params_row', 'wn_mol_sample'}
    assert set(tg.ENTRIES) == set(w)


OK, BAD_SHAPE, UNSUPPORTED, MISALIGNED, NULL = 0, -1, -2, -3, -5


def test_the_entries_own_checks(hip_lib):
    """Every refusal comes back before any launch (no device here)."""
    import ctypes
    buf = (ctypes.c_double * 1024)()
    a = ctypes.addressof(buf)
    assert a % 16 == 0
    L = hip_lib
    assert L.wn_mol_score_scratch_floats(10) == 20
    assert L.wn_mol_score_scratch_floats(0) == 0
    assert L.wn_mol_quantize(None, None, a, a, 1, 8, None) == NULL
    assert L.wn_mol_quantize(a, None, a, a, 0, 8, None) == BAD_SHAPE
    assert L.wn_mol_quantize(a, None, a, a, 2 ** 16, 2 ** 15, None) == BAD_SHAPE
    assert L.wn_mol_quantize(a, None, a + 2, a, 1, 8, None) == MISALIGNED

    def loss(lg=a, ld=12, lv=a, dl=None, parts=a, B=1, T=4, K=4, lsm=-14.0):
        return L.wn_mol_loss(lg, ld, lv, None, None, None, dl, parts, B, T, K,
                             lsm, None)
    assert loss(lg=None) == NULL and loss(lv=None) == NULL
    assert loss(parts=None) == NULL
    assert loss(T=0) == BAD_SHAPE and loss(K=0) == BAD_SHAPE
    assert loss(K=33, ld=108) == BAD_SHAPE
    assert loss(lsm=-0.5) == BAD_SHAPE and loss(lsm=-40.0) == BAD_SHAPE
    assert loss(lsm=float('nan')) == BAD_SHAPE
    assert loss(K=5, ld=12) == UNSUPPORTED          # Kp = 8: 24 columns
    assert loss(ld=14) == UNSUPPORTED
    assert loss(lg=a + 4) == MISALIGNED and loss(dl=a + 8) == MISALIGNED

    def score(lg=a, ld=12, clip=a, cnt=a, scr=a, K=4):
        return L.wn_mol_score(lg, ld, a, None, None, None, clip, cnt, scr, 1,
                              4, K, -14.0, None)
    assert score(clip=None) == NULL and score(scr=None) == NULL
    assert score(K=40) == BAD_SHAPE and score(ld=8) == UNSUPPORTED
    assert score(clip=a + 4) == MISALIGNED
    assert L.wn_mol_params_row(None, 4, -14.0, a, None) == NULL
    assert L.wn_mol_params_row(a, 0, -14.0, a, None) == BAD_SHAPE
    assert L.wn_mol_params_row(a, 4, 0.0, a, None) == BAD_SHAPE
    assert L.wn_mol_sample(a, a, None, 1.0, a, a, 1, 4, None) == NULL
    assert L.wn_mol_sample(a, a, a, -1.0, a, a, 1, 4, None) == BAD_SHAPE
    assert L.wn_mol_sample(a, a, a, float('inf'), a, a, 1, 4, None) == BAD_SHAPE
    assert L.wn_mol_sample(a, a, a, 1.0, a, a, 0, 4, None) == BAD_SHAPE
    assert L.wn_mol_sample(a, a + 4, a, 1.0, a, a, 1, 4, None) == MISALIGNED
