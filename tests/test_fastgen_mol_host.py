"""Batched fast generation for mixture-of-logistics models, host side (no
device): the binding table against include/wavenet_fastgen_mol.h, the guard
file's ENTRIES against the header, argument errors raised before any device
or library call, the entries' own refusals, and generate.py's --fast_mixture
flag errors.  The history-ring statement of the causal layer
(tests/fastgen_mol_ref.py) is held against the float64 network's causal
convolution: that checks the restatement in the header's words, test
infrastructure only -- it runs no kernel, and the kernel is held to the
float64 network itself in tests/test_gpu_fastgen_mol.py."""
import glob
import os
import re

import numpy as np
import pytest
import torch

import fastgen_mol_ref as FR
from util import ROOT, TINY, cfg_with, model_kwargs

HEADER = 'wavenet_fastgen_mol.h'
NAMES = {'wn_fastgen_mol_init', 'wn_fastgen_mol_pre', 'wn_fastgen_mol_step',
         'wn_fastgen_mol_finish', 'wn_fastgen_mol_restart'}


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
    assert set(decl) == NAMES
    assert set(_lib.FASTGEN_MOL_SIGNATURES) == set(decl)
    ctype = {'int': _lib.c_int, 'long': _lib.c_long, 'float': _lib.c_float,
             'double': _lib.c_double}
    for name, (res, params) in decl.items():
        want = [_lib.P if '*' in p else ctype[p.split()[0]] for p in params]
        assert _lib.FASTGEN_MOL_SIGNATURES[name] == (ctype[res], want), name
    for path in glob.glob(os.path.join(ROOT, 'include', '*.h')):
        other = os.path.basename(path)
        if other != HEADER:
            assert not set(decl) & set(_declarations(other)), other
    for name, table in vars(_lib).items():
        if name.endswith('SIGNATURES') and name != 'FASTGEN_MOL_SIGNATURES':
            assert not set(decl) & set(table), name


def test_load_binds_the_table(hip_lib):
    from wavenet import _lib
    for name, (res, args) in _lib.FASTGEN_MOL_SIGNATURES.items():
        fn = getattr(hip_lib, name)
        assert fn.restype is res and fn.argtypes == args, name


def test_every_writing_entry_of_the_header_is_guarded():
    import test_gpu_guard_fastgen_mol as tg
    w = {k: [p for p in v[1] if '*' in p and not p.startswith('const ')
             and not re.search(r'\bstream$', p)]
         for k, v in _declarations(HEADER).items()}
    w = {k: v for k, v in w.items() if v}
    assert set(w) == NAMES
    assert w['wn_fastgen_mol_pre'] == ['float* pre']
    assert w['wn_fastgen_mol_restart'] == ['float* state', 'int32_t* hist',
                                           'int32_t* origins']
    assert set(tg.ENTRIES) == set(w)


# ------------------------------------------------------- argument errors
def _net(**kw):
    from wavenet import WaveNetModel
    cfg = cfg_with(TINY, batch_size=1, scalar_input=True,
                   initial_filter_width=4)
    args = model_kwargs(cfg)
    args.update(kw)
    return WaveNetModel(device='cpu', **args)


@pytest.fixture
def untouched(hip_lib, monkeypatch):
    """Models on the host; from here on no library entry and no device."""
    from wavenet import _lib
    nets = dict(mix=_net(output_mixture=4), plain=_net(),
                wide=_net(output_mixture=4, initial_filter_width=33),
                ok32=_net(output_mixture=4, initial_filter_width=32))
    monkeypatch.setattr(_lib, 'call',
                        lambda *a: pytest.fail('library called: %s' % a[0]))
    monkeypatch.setattr(_lib, 'load', lambda: pytest.fail('library touched'))
    monkeypatch.setattr(_lib, 'require_gpu',
                        lambda: pytest.fail('device touched'))
    monkeypatch.setattr(torch.Tensor, 'cuda',
                        lambda *a, **k: pytest.fail('device touched'))
    return nets


def test_not_a_mixture_model_is_a_value_error(untouched):
    net = untouched['plain']
    for call in (lambda: net.generate_mixture_batch(4, [1]),
                 lambda: net.continue_mixture_batch(4, [0], [1]),
                 lambda: net.generate_mixture(4),
                 lambda: net.continue_mixture(4, 0)):
        with pytest.raises(ValueError, match='without output_mixture'):
            call()


def test_initial_filter_width_limit_names_itself(untouched):
    with pytest.raises(NotImplementedError, match=r'1 to 32.*has 33'):
        untouched['wide'].generate_mixture_batch(4, [1])
    with pytest.raises(NotImplementedError, match=r'1 to 32.*has 33'):
        untouched['wide'].generate_mixture(4)


@pytest.mark.parametrize('levels,what', [
    ([[1, 2], [3]], 'seed_levels must be'),
    (np.zeros((2, 2, 2), np.int32), 'seed_levels must be'),
    (np.zeros((3, 4), np.int32), '3 rows for 2 streams'),
    (np.zeros((2, 0), np.int32), 'at least one level'),
    ([0.5, 0.25], 'seed_levels must be'),
    ([0, 65536], '0 .. 65535'),
    ([-1, 5], '0 .. 65535'),
])
def test_bad_seed_levels(untouched, levels, what):
    with pytest.raises(ValueError, match=what):
        untouched['mix'].generate_mixture_batch(4, [1, 2], levels)


@pytest.mark.parametrize('restart', [[2], [-1], [0, 0], [0.5], [True],
                                     [[0]]])
def test_bad_restart_lists(untouched, restart):
    with pytest.raises(ValueError, match='restart must'):
        untouched['mix'].continue_mixture_batch(4, [0, 1], [1, 2],
                                                restart=restart)


def test_other_argument_errors(untouched):
    net = untouched['mix']
    for t in (-0.5, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='temperature'):
            net.generate_mixture_batch(4, [1], temperature=t)
        with pytest.raises(ValueError, match='temperature'):
            net.continue_mixture_batch(4, [0], [1], temperature=t)
    with pytest.raises(ValueError,
                       match='generate_mixture_batch takes 1 to 256 streams'):
        net.generate_mixture_batch(4, [])
    with pytest.raises(ValueError, match='1 to 256 streams'):
        net.generate_mixture_batch(4, list(range(257)))
    with pytest.raises(ValueError, match='num_samples'):
        net.generate_mixture_batch(-1, [1])
    with pytest.raises(ValueError, match='reserve_steps'):
        net.generate_mixture_batch(4, [1], reserve_steps=-2)
    with pytest.raises(ValueError, match='last_samples has 1'):
        net.continue_mixture_batch(4, [0], [1, 2])
    with pytest.raises(ValueError, match='last_levels must lie'):
        net.continue_mixture_batch(4, [0, 70000], [1, 2])
    with pytest.raises(ValueError, match='global_condition has 3 ids'):
        net.generate_mixture_batch(4, [1, 2], global_condition=[0, 1, 2])
    # the one-hot entry points keep refusing such a model
    for call in (lambda: net.generate(4), lambda: net.generate_batch(4, [1])):
        with pytest.raises(NotImplementedError, match='follow-up'):
            call()


def test_follow_up_names_what_remains():
    from wavenet import mol
    for word in ('follow-up', '--fast_generation false', '--fast_mixture',
                 'persistent', 'bulk synthesis', 'evaluate.py --synthesis',
                 'softmax'):
        assert word in mol.FOLLOW_UP, word


# --------------------------------------------- the history-ring tap rule
@pytest.mark.parametrize('K0', [1, 2, 3, 4, 32])
def test_ring_rule_is_the_networks_causal_convolution(K0):
    """150 steps (more than two wraps of the 64 slots), the first `reach`
    steps -- where taps fall in front of the sequence -- included, against
    the causal convolution tests/mol_ref.py's forward runs."""
    from oracle.torch_graph import causal_conv
    from wavenet import mol
    rng = np.random.default_rng(K0)
    n, C = 150, 7
    levels = rng.integers(0, 65536, n)
    levels[:4] = [0, 1, 65534, 65535]
    W = rng.standard_normal((K0, C))
    x = torch.as_tensor(mol.centres(levels).astype(np.float64))
    want = causal_conv(x.reshape(1, n, 1),
                       torch.as_tensor(W).reshape(K0, 1, C), 1)[0].numpy()
    got = FR.ring_causal(levels, W)
    assert got.shape == want.shape == (n, C)
    reach = (K0 - 1) + (K0 - 1) // 2
    assert reach < FR.SLOTS
    for t in range(n):
        assert np.abs(got[t] - want[t]).max() <= 1e-12 * max(
            1.0, np.abs(want[t]).max()), t
    if K0 > 2:
        # the newest (K0 - 1) / 2 levels are not read: step 0 sees nothing
        assert not got[:(K0 - 1) // 2].any()
        assert got[(K0 - 1) // 2].any()
    # the float32 centre the kernels form is mol.centres'
    assert FR.centre32(12345) == float(mol.centres([12345])[0])


# ------------------------------------------------ the entries' own checks
OK, BAD_SHAPE, UNSUPPORTED, MISALIGNED, NULL = 0, -1, -2, -3, -5


def test_the_entries_own_checks(hip_lib):
    """Every refusal comes back before any launch (no device here)."""
    import ctypes
    buf = (ctypes.c_double * 1024)()
    a = ctypes.addressof(buf)
    assert a % 16 == 0
    L = hip_lib
    assert L.wn_fastgen_mol_init(None, 64, a, a, 1, None) == NULL
    assert L.wn_fastgen_mol_init(a, 64, a, None, 1, None) == NULL
    assert L.wn_fastgen_mol_init(a, 64, a, a, 0, None) == BAD_SHAPE
    assert L.wn_fastgen_mol_init(a, 64, a, a, 257, None) == UNSUPPORTED
    assert L.wn_fastgen_mol_init(a, 0, a, a, 1, None) == BAD_SHAPE
    assert L.wn_fastgen_mol_init(a + 4, 64, a, a, 1, None) == MISALIGNED
    assert L.wn_fastgen_mol_init(a, 64, a, a + 2, 1, None) == MISALIGNED

    def pre(layer0=a, L_=2, B=1, pre_=a, ring=None, R=0, stride=0):
        return L.wn_fastgen_mol_pre(layer0, 5216, None, 0, a, L_, B, a, a,
                                    pre_, ring, R, stride, None)
    assert pre(layer0=None) == NULL and pre(pre_=None) == NULL
    assert pre(L_=0) == BAD_SHAPE and pre(L_=65) == UNSUPPORTED
    assert pre(B=0) == BAD_SHAPE and pre(B=300) == UNSUPPORTED
    assert pre(ring=a, R=0) == BAD_SHAPE and pre(ring=a, R=3, stride=32) \
        == BAD_SHAPE
    assert pre(pre_=a + 2) == MISALIGNED

    def step(K0=4, K=4, B=1, hist=a, seeds=a, lsm=-14.0, S=32, causal=a,
             ring=None, R=0):
        return L.wn_fastgen_mol_step(
            causal, K0, a, 5216, a, None, a, None, a, None, None, 0, a, 2, S,
            K, B, a, a, hist, a, a, seeds, None, 0, lsm, a, a, a, a, a, ring,
            R, 0, None, None)
    assert step(causal=None) == NULL and step(hist=None) == NULL
    assert step(seeds=None) == NULL
    assert step(K0=0) == BAD_SHAPE and step(K0=33) == BAD_SHAPE
    assert step(K=0) == BAD_SHAPE and step(K=33) == BAD_SHAPE
    assert step(B=0) == BAD_SHAPE and step(B=257) == UNSUPPORTED
    assert step(lsm=-0.5) == BAD_SHAPE and step(lsm=float('nan')) == BAD_SHAPE
    assert step(S=513) == UNSUPPORTED
    assert step(ring=a, R=0) == BAD_SHAPE
    assert step(hist=a + 2) == MISALIGNED and step(seeds=a + 4) == MISALIGNED

    def finish(K=4, B=1, cur=a, seeds=a, lg=a, lsm=-14.0):
        return L.wn_fastgen_mol_finish(K, lsm, B, cur, a, a, seeds, None, lg,
                                       None, None)
    assert finish(cur=None) == NULL and finish(lg=None) == NULL
    assert finish(K=0) == BAD_SHAPE and finish(K=40) == BAD_SHAPE
    assert finish(B=0) == BAD_SHAPE and finish(B=257) == UNSUPPORTED
    assert finish(lsm=0.0) == BAD_SHAPE
    assert finish(seeds=a + 4) == MISALIGNED and finish(cur=a + 1) == MISALIGNED

    def restart(state=a, L_=2, B=1, hist=a, flags=a):
        return L.wn_fastgen_mol_restart(state, a, L_, B, a, hist, a, flags,
                                        None)
    assert restart(state=None) == NULL and restart(hist=None) == NULL
    assert restart(flags=None) == NULL
    assert restart(L_=0) == BAD_SHAPE and restart(L_=65) == UNSUPPORTED
    assert restart(B=0) == BAD_SHAPE and restart(B=257) == UNSUPPORTED
    assert restart(state=a + 4) == MISALIGNED
    assert restart(hist=a + 2) == MISALIGNED


# ------------------------------------------------------------ command line
@pytest.mark.parametrize('argv,words', [
    (['--fast_mixture', 'true', '--fast_generation', 'false'],
     ('--fast_mixture', '--fast_generation false')),
    (['--fast_mixture', 'true', '--top_k', '5'],
     ('--fast_mixture', '--top_k / --top_p')),
    (['--fast_mixture', 'true', '--top_p', '0.5'],
     ('--fast_mixture', '--top_k / --top_p')),
    (['--fast_mixture', 'true', '--lc_wav_dir', 'd', '--wav_out_dir', 'o'],
     ('--fast_mixture', '--lc_wav_dir', 'follow-up')),
    (['--fast_mixture', 'perhaps'], ('--fast_mixture',)),
])
def test_fast_mixture_flag_errors(argv, words, capsys):
    import generate
    with pytest.raises(SystemExit) as e:
        generate.get_arguments(['ckpt'] + argv)
    err = capsys.readouterr().err
    assert e.value.code == 2 and all(w in err for w in words), err


def test_fast_mixture_flag_defaults():
    import generate
    a = generate.get_arguments(['ckpt'])
    assert a.fast_mixture is False and a.fast_generation is True
    a = generate.get_arguments(['ckpt', '--fast_mixture', 'true', '--clips',
                                '3', '--save_every', '10'])
    assert a.fast_mixture is True and a.clips == 3
