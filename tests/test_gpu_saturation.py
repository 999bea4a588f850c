"""tanh, sigmoid and softmax sites of the HIP kernels against float64 where
they SATURATE: gate weights times a gain, biases that force tanh = +-1, sigmoid
= 0 / 1 exactly and a sigmoid of 1e-26 (tests/sat_ref.py; the CPU half,
tests/test_saturation_host.py, asserts that every case reaches the regime).

Nothing is chained: every layer is checked from the DEVICE's own input planes
(x_l, dZ_l, dx_{l+1}), so the comparison stays well conditioned at any gain.
Every bound is measured on the same inputs with a float32 numpy evaluation of
the same block (or the float32 oracle), never with the code under test:

  forward planes       4 x max|f32 - f64| + 1e-6 (16 ulp of 1.0: the device's
                       exp -> add -> rcp -> fma chain, which libm does not share)
  layer gradients      per variable, in its norm: 8 x |f32 - f64| / |f64|, and
                       never above test_gpu_stack.py's 1e-4
  end to end           test_gpu_model.check_grads with 4 x the float32 oracle's
                       own error, computed here
  fast generation      max(1e-5, 4 x IncrementalGenerator(float32)'s error)
  cross-entropy        4 x a float32 numpy evaluation's error

and each test asserts which launch ran.  Observed device / float32 error ratios
go to saturation_errors.json, beside the other parity tests' error logs.
"""
import contextlib

import numpy as np
import pytest
import torch

import sat_ref as S
from util import O, model_kwargs, tree_to_numpy, flat_named, \
    oracle_grads_at_device_kinks

pytestmark = pytest.mark.gpu

_RATIOS = {}     # path -> {quantity: (device error, float32 reference error)}


def _log(path, what, dev, ref):
    cur = _RATIOS.setdefault(path, {}).get(what)
    if cur is None or dev * (cur[1] + 1e-300) > cur[0] * (ref + 1e-300):
        _RATIOS[path][what] = (float(dev), float(ref))


@pytest.fixture(scope='module', autouse=True)
def _dump_ratios():
    yield
    if not _RATIOS:
        return
    worst = {}
    for path, qs in _RATIOS.items():
        ratio, what = max(((dev / ref, w) for w, (dev, ref) in qs.items()
                           if ref > 0), default=(0.0, ''))
        worst[path] = dict(ratio=ratio, what=what)
    # (where test_gpu_fullsize.py keeps its error log)
    from test_gpu_fullsize import _log as log_json
    log_json('worst_ratio_per_path', worst, 'saturation_errors.json')
    log_json('all', _RATIOS, 'saturation_errors.json')


@contextlib.contextmanager
def _spy(net):
    """Names of the library entry points called meanwhile, and a copy of the
    dL/dx plane(s) every per-layer backward launch wrote (those kernels
    ping-pong between two planes; the persistent launch keeps every layer's
    with `stack_bwd_keep_dx`)."""
    from wavenet import _lib
    names, dxs = [], []
    real = _lib.call, _lib.call_timed
    slot = {'wn_layer_bwd2': 5, 'wn_layer_bwd_k': 3, 'wn_layer_bwd_blk': 5}

    def grab(name, args):
        names.append(name)
        i = slot.get(name)
        if i is None or args[i] is None:
            return
        for ws in net._ws.values():
            if ws.training:
                dxs.extend(ws.dx[p].clone() for p in range(2)
                           if ws.dx[p].data_ptr() == args[i])

    def call(name, *args):
        real[0](name, *args)
        grab(name, args)

    def call_timed(name, args, flops, events):
        real[1](name, args, flops, events)
        grab(name, args)
    _lib.call, _lib.call_timed = call, call_timed
    try:
        yield names, dxs
    finally:
        _lib.call, _lib.call_timed = real


def _model(cfg, var):
    from wavenet import WaveNetModel
    kw = {}
    if cfg.get('local_condition_channels'):
        kw['local_condition_channels'] = cfg['local_condition_channels']
    net = WaveNetModel(**model_kwargs(cfg), **kw)
    net.load_nested(var)
    return net


# --------------------------------------------------------- training launches
def _variant(rows, waves):
    from wavenet._lib import stack_variant
    return stack_variant(rows=rows, waves=waves)


# path -> (case, how to select it, entry points that must / must not run)
PATHS = {
    'rows32': ('mid', dict(variant=(32, 0)), ['wn_stack_fwd', 'wn_stack_bwd'], []),
    'rows32_w8': ('mid', dict(variant=(32, 8)), ['wn_stack_fwd', 'wn_stack_bwd'], []),
    'rows16_w4': ('mid', dict(variant=(16, 4)), ['wn_stack_fwd', 'wn_stack_bwd'], []),
    'rows16_w8': ('mid', dict(variant=(16, 8)), ['wn_stack_fwd', 'wn_stack_bwd'], []),
    'perlayer': ('mid', dict(stack=False), ['wn_layer_fwd', 'wn_layer_bwd2'],
                 ['wn_stack_fwd', 'wn_stack_bwd']),
    'fused_skip': ('mid_S512', dict(), ['wn_stack_fwd_skip', 'wn_stack_bwd'],
                   ['wn_stack_fwd']),
    'generic': ('mid', dict(generic=True), ['wn_layer_fwd_k', 'wn_layer_bwd_k'],
                ['wn_stack_fwd', 'wn_layer_fwd', 'wn_layer_bwd2']),
    'k3': ('mid_k3', dict(), ['wn_layer_fwd_k', 'wn_layer_bwd_k'],
           ['wn_stack_fwd', 'wn_layer_fwd']),
    'r64': ('r64', dict(), ['wn_layer_fwd_blk', 'wn_dense_planes_gate',
                            'wn_layer_bwd_blk'], []),
    'r64_unfused': ('r64', dict(fuse_gate=False),
                    ['wn_layer_fwd_blk', 'wn_layer_bwd_k', 'wn_layer_bwd_blk'],
                    ['wn_dense_planes_gate']),
    'lc': ('mid_lc', dict(), ['wn_stack_fwd_lc', 'wn_stack_bwd_lc'],
           ['wn_stack_fwd', 'wn_stack_bwd']),
    'T20': ('mid_T20', dict(), ['wn_stack_fwd', 'wn_stack_bwd'], []),
    'T20_rows32': ('mid_T20', dict(variant=(32, 0)),
                   ['wn_stack_fwd', 'wn_stack_bwd'], []),
}
_TRAIN = [(p, g) for p, v in PATHS.items() for g in S.CASES[v[0]][2]]
_TRAIN_IDS = ['%s-g%g' % a for a in _TRAIN]
_RUNS = {}


def _planes(t, L, CB, B, T, C):
    """[L * CB][N][32] device planes -> float64 [L][B, T, C]."""
    a = t.detach().cpu().numpy().astype(np.float64).reshape(L, CB, B, T, 32)
    return a.transpose(0, 2, 3, 1, 4).reshape(L, B, T, CB * 32)[..., :C]


def _run(hip_lib, path, gain):
    """One training step on `path`; the device's planes and gradients, and the
    float64 / float32 restatements of every layer from those planes."""
    if (path, gain) in _RUNS:
        return _RUNS[path, gain]
    case, how, must, must_not = PATHS[path]
    cfg, T = S.CASES[case][:2]
    B, L, K = cfg['batch_size'], len(cfg['dilations']), cfg['filter_width']
    R, D = cfg['residual_channels'], cfg['dilation_channels']
    net = _model(cfg, S.saturated_variables(cfg, gain))
    if 'variant' in how:
        net.stack_variant = _variant(*how['variant'])
    if how.get('stack') is False:
        net.stack_fwd = net.stack_bwd = False
    if how.get('generic'):
        net.generic_layers = True
    if how.get('fuse_gate') is False:
        net.wide_fuse_gate = False
    net.stack_bwd_keep_dx = True
    _, audio, lc = S.case_inputs(case)
    with _spy(net) as (names, dxs):
        loss = net.loss(audio, local_condition_batch=lc) if lc is not None \
            else net.loss(audio)
        torch.cuda.synchronize()
    assert np.isfinite(float(loss))
    net.check_device_errors()
    ws = [w for w in net._ws.values() if w.training and w.T == T][0]
    # ---- the launches this path is about are the ones that ran
    for n in must:
        assert n in names, (path, n, sorted(set(names)))
    for n in must_not:
        assert n not in names, (path, n)
    sp = net._step_path(ws, True)
    if 'variant' in how:
        rows = how['variant'][0]
        assert ws.stack_rows == rows and ws.stack_bwd
        assert hip_lib.wn_stack_tile_rows(B, T, ws.stack_variant) == rows
        assert (sp.fwd, sp.bwd) == ('stack', 'stack')
        assert ws.stack_variant == _variant(*how['variant'])
    elif path == 'perlayer':
        assert (sp.fwd, sp.bwd) == ('layer', 'layer2')
    elif path == 'fused_skip':
        assert hip_lib.wn_stack_fwd_skip_ok(B, T, cfg['skip_channels'], 0) == 1
        assert (sp.fwd, sp.bwd) == ('stack_skip', 'stack')
        assert getattr(ws, 'skimg', None) is not None
    elif path in ('generic', 'k3'):
        assert (sp.fwd, sp.bwd) == ('layer_k', 'layer_k') and net.KW == K
    elif path.startswith('r64'):
        assert (sp.fwd, sp.bwd) == ('blocked', 'blocked') and net.CB == 2
    elif path == 'lc':
        assert (sp.fwd, sp.bwd) == ('stack_lc', 'stack_lc') and ws.stack_rows == 32
    else:
        assert (sp.fwd, sp.bwd) == ('stack', 'stack')
        assert ws.stack_rows == hip_lib.wn_stack_tile_rows(B, T, 0)
    # ---- the device's planes
    CB = net.CB
    r = dict(cfg=cfg, B=B, T=T, L=L, K=K, path=path,
             X=_planes(ws.X, L, CB, B, T, R), Z=_planes(ws.Z, L, CB, B, T, D),
             SG=_planes(ws.SG, L, CB, B, T, D),
             TH=None if ws.TH is None else _planes(ws.TH, L, CB, B, T, D),
             dZ=_planes(ws.dZ, L, CB, B, T, D),
             grads=tree_to_numpy(net.gradients),
             flat_grads=net.grads.detach().cpu().numpy(),
             h1=ws.h1.detach().cpu().numpy().astype(np.float64).reshape(B, T, -1))
    dil = cfg['dilations']
    if sp.bwd.startswith('stack'):
        assert ws.DX.shape[0] == L                  # every layer's dx kept
        own, q = _planes(ws.DX, L, 1, B, T, R), _planes(ws.DQ, L, 1, B, T, R)
        # DX[l] holds dx_l without the tap's term, which sits in DQ[l] at the
        # rows d_l later; dx_0 is completed in place
        r['dx'] = [own[0]] + [own[l] + S.unshift(q[l], int(dil[l]))
                              for l in range(1, L)]
    else:
        assert len(dxs) == L, (path, len(dxs))      # one launch per layer,
        r['dx'] = [_planes(t, 1, CB, B, T, R)[0]    # last layer first
                   for t in reversed(dxs)]
    lc_add = lc_da = None
    if lc is not None:
        f = lambda t: t.detach().cpu().numpy().astype(np.float64).reshape(B, T, L, 2, 32)
        lc_add, lc_da = f(ws.lc_add), f(ws.lc_da)
        r['lc_da'] = lc_da
    # ---- float64 and float32 restatements of every layer from those planes,
    # on the weights the device holds
    var = tree_to_numpy(net.variables)
    r['var'] = var
    r['fwd'], r['bwd'] = [], []
    for l in range(L):
        blk = S.block_of(var, l, dil, K)
        x = r['X'][l]
        xs = S.shifted_taps(x, blk['shifts'])
        add = None if lc_add is None else (lc_add[:, :, l, 0, :D], lc_add[:, :, l, 1, :D])
        dxn = r['dx'][l + 1] if l + 1 < L else None
        r['fwd'].append(tuple(S.layer_forward(x, xs, blk, S.bias_of(var, l), add, dt)
                              for dt in (np.float64, np.float32)))
        r['bwd'].append(tuple(S.layer_backward(x, xs, r['dZ'][l], dxn, blk,
                                               S.bias_of(var, l), add, dt)
                              for dt in (np.float64, np.float32)))
    _RUNS[path, gain] = r
    return r


@pytest.mark.parametrize('path,gain', _TRAIN, ids=_TRAIN_IDS)
def test_forward_planes_per_layer(hip_lib, path, gain):
    """tanh (where stored), sigmoid, z and x_{l+1} of every layer against
    layer_forward(float64) evaluated from the device's x_l."""
    r = _run(hip_lib, path, gain)
    L, tag = r['L'], '%s-g%g' % (path, gain)
    zero_rows = 0
    for l in range(L):
        f64, f32 = r['fwd'][l]
        dev = dict(SG=(r['SG'][l], 1), Z=(r['Z'][l], 2))
        if r['TH'] is not None:
            dev['TH'] = (r['TH'][l], 0)
        if l + 1 < L:
            dev['X'] = (r['X'][l + 1], 3)
        for name, (got, i) in dev.items():
            assert np.isfinite(got).all(), (tag, l, name)
            e32 = np.abs(f32[i].astype(np.float64) - f64[i]).max()
            err = np.abs(got - f64[i]).max()
            _log(tag, 'fwd/' + name, err, e32 + 0.25e-6)
            assert err <= 4.0 * e32 + 1e-6, (tag, l, name, err, e32)
        th, sg, z = f64[0], f64[1], f64[2]
        SG, Z = r['SG'][l], r['Z'][l]
        # exact range, exact saturation
        assert (SG >= 0).all() and (SG <= 1).all() and (np.abs(Z) <= 1).all(), (tag, l)
        assert (SG[sg < 1e-46] == 0).all() and (Z[sg < 1e-46] == 0).all(), (tag, l)
        assert (SG[sg == 1.0] == 1).all(), (tag, l)
        assert (Z[th == 1.0] == SG[th == 1.0]).all(), (tag, l)
        assert (Z[th == -1.0] == -SG[th == -1.0]).all(), (tag, l)
        zero_rows += int((sg < 1e-46).sum())
        if r['TH'] is not None:
            TH = r['TH'][l]
            assert (np.abs(TH) <= 1).all(), (tag, l)
            assert (TH[th == 1.0] == 1).all() and (TH[th == -1.0] == -1).all(), (tag, l)
    # the planted channel: sigmoid exactly 0 in every row, so z exactly 0
    assert (r['SG'][1][..., 0] == 0).all() and (r['Z'][1][..., 0] == 0).all()
    assert (r['SG'][1][..., 1] == 1).all()
    assert zero_rows >= r['B'] * r['T']
    if path == 'fused_skip':
        # the skip sum of the same launch: h1 = relu(sum_l z_l Ws_l + sum_l bs_l)
        hs = []
        for dt in (np.float64, np.float32):
            v = O.cast_variables(r['var'], dt)
            tot = sum(r['Z'][l].astype(dt) @ v['dilated_stack'][l]['skip'][0] +
                      v['dilated_stack'][l]['skip_bias'] for l in range(L))
            assert tot.dtype == dt
            hs.append(np.maximum(tot, 0).astype(np.float64))
        e32 = np.abs(hs[1] - hs[0]).max()
        err = np.abs(r['h1'] - hs[0]).max()
        _log(tag, 'fwd/h1', err, e32 + 0.25e-6)
        assert np.isfinite(r['h1']).all() and err <= 4.0 * e32 + 1e-6, (err, e32)


@pytest.mark.parametrize('path,gain', _TRAIN, ids=_TRAIN_IDS)
def test_layer_gradients_per_variable(hip_lib, path, gain):
    """Every layer's weight / bias gradients and dL/dx_l against
    layer_backward(float64) fed the device's x_l, dZ_l and dx_{l+1}, each in
    the norm of the variable; on the LC launch also the stored da_f | da_g."""
    r = _run(hip_lib, path, gain)
    L, K, tag = r['L'], r['K'], '%s-g%g' % (path, gain)
    assert np.isfinite(r['flat_grads']).all()
    for l in range(L):
        b64, b32 = r['bwd'][l]
        dev = S.device_sections(r['grads'], l, K, l == L - 1)
        dev['dx'] = r['dx'][l]
        if 'lc_da' in r:
            D = r['cfg']['dilation_channels']
            dev['da_f'] = r['lc_da'][:, :, l, 0, :D]
            dev['da_g'] = r['lc_da'][:, :, l, 1, :D]
        assert set(b64) - set(dev) <= {'da_f', 'da_g'}, (set(b64), set(dev))
        for name, got in dev.items():
            ref = b64[name]
            assert got.shape == ref.shape, (name, got.shape, ref.shape)
            assert np.isfinite(got).all(), (tag, l, name)
            n = np.linalg.norm(ref)
            if n == 0:            # (no row reaches the tap: T <= shift)
                assert not got.any(), (tag, l, name)
                continue
            e32 = np.linalg.norm(b32[name].astype(np.float64) - ref) / n
            err = np.linalg.norm(got - ref) / n
            _log(tag, 'bwd/' + name, err, e32)
            assert err <= min(8.0 * e32, 1e-4), (tag, l, name, err, e32)
    # the channel whose sigmoid is exactly 0 in every row gets no gradient
    assert (r['SG'][1][..., 0] == 0).all()
    cur = r['grads']['dilated_stack'][1]
    for k in ('filter', 'gate'):
        assert not cur[k][..., 0].any(), (tag, k)
    assert cur['filter_bias'][0] == 0 and cur['gate_bias'][0] == 0, tag


# ------------------------------------------------------------- end to end
@pytest.mark.parametrize('case', ['tiny', 'mid'])
def test_loss_and_gradients_vs_oracle_saturated(hip_lib, monkeypatch, case):
    """test_gpu_model.test_loss_and_gradients_vs_oracle's rule at gain 3:
    check_grads itself, with 4 x the float32 oracle's own error against
    float64 (computed here, on the device's ReLU decisions) where that is
    above GRAD_REL; the kink tolerance widened the same way."""
    import test_gpu_model as M
    cfg, T = S.CASES[case][:2]
    B = cfg['batch_size']
    net = _model(cfg, S.saturated_variables(cfg, 3.0))
    var = tree_to_numpy(net.variables)
    _, audio, _ = S.case_inputs(case)
    loss = net.loss(audio)
    torch.cuda.synchronize()
    ws = list(net._ws.values())[0]
    assert ws.stack_rows == hip_lib.wn_stack_tile_rows(B, T, 0) and ws.stack_bwd
    with np.errstate(over='ignore'):      # (exp(+large) = inf: a sigmoid of 0)
        l64, c64 = O.loss(cfg, var, audio, dtype=np.float64, keep=True)
        l32, c32 = O.loss(cfg, var, audio, dtype=np.float32, keep=True)
        e_total = float(np.abs(c32['total'] - c64['total']).max())
        ref_loss, ref_g, c, flips = oracle_grads_at_device_kinks(
            net, cfg, var, audio, kink_tol=max(2e-5, 4.0 * e_total), cache=c64)
        S_ = cfg['skip_channels']
        masks = dict(total=(ws.h1 > 0).cpu().numpy().reshape(B, T, S_),
                     c1=(ws.h2 > 0).cpu().numpy().reshape(B, T, S_))
        _, g32 = O.loss_and_grads(cfg, var, audio, dtype=np.float32,
                                  relu_masks=masks)
    # (relative to the variable's largest entry, as check_grads measures; the
    # last layer's dense conv has no gradient at all)
    rel = lambda a, b: float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
    e32 = {n: rel(a, b)
           for (n, a), (_, b) in zip(flat_named(g32), flat_named(ref_g))}
    monkeypatch.setattr(M, '_fp32_oracle_error', lambda tag: e32)
    tag = 'e2e_%s-g3' % case
    got = tree_to_numpy(net.gradients)
    for (n, a), (_, b) in zip(flat_named(got), flat_named(ref_g)):
        assert np.isfinite(a).all(), n
        _log(tag, n.split('wavenet/')[-1], rel(a, b),
             max(e32[n], M.GRAD_REL / 4))
    assert abs(float(loss) - ref_loss) < max(M.TOL, 4.0 * abs(float(l32) - l64))
    M.check_grads(net, ref_g, tag='saturated_' + case)
    M.check_planes(net, cfg, c, B, T)


# -------------------------------------------------------- fast generation
_GEN_REF = {}


def _gen_ref(case, gain, var, stream=0):
    """(codes [n], float64 and float32 reference probabilities [n - 1, Q]) of
    a case's teacher-forced trace: oracle.IncrementalGenerator, or for an LC
    model (which the oracle does not know) sat_ref.forward_chain."""
    key = (case, gain, stream)
    if key not in _GEN_REF:
        cfg = S.CASES[case][0]
        codes, _, lc = S.case_inputs(case, stream)
        ps = []
        for dt in (np.float64, np.float32):
            if lc is None:
                gen = O.IncrementalGenerator(cfg, var, dtype=dt)
                with np.errstate(over='ignore'):
                    ps.append(np.stack([gen.step(int(c)) for c in codes[0, :-1]]))
            else:
                lg = S.forward_chain(cfg, var, codes[:, :-1], lc[:, :-1], dt)['logits']
                assert lg.dtype == dt
                ps.append(S.softmax64(lg[0]))
        _GEN_REF[key] = (codes[0], lc, ps[0].astype(np.float64),
                         ps[1].astype(np.float64))
    return _GEN_REF[key]


def _check_probs(tag, p, ref):
    codes, _, p64, p32 = ref
    p = np.asarray(p, np.float64)
    assert p.shape == p64.shape, (p.shape, p64.shape)
    assert np.isfinite(p).all() and (p >= 0).all(), tag
    assert np.abs(p.sum(-1) - 1).max() <= 1e-6, tag
    e32 = np.abs(p32 - p64).max()
    err = np.abs(p - p64).max(axis=1)
    _log(tag, 'proba', err.max(), max(e32, 0.25e-5))
    assert err.max() <= max(1e-5, 4.0 * e32), (tag, int(err.argmax()), err.max(), e32)


def _gen_paths(net, paths, codes, lc, tag):
    out = {}
    for path in paths:
        net.fastgen_multi_cu = path != 'single'
        net.fastgen_persistent = path == 'persist'
        net.fastgen_graph_steps = 50            # graph capture and replay
        with _spy(net) as (names, _):
            io, p = net.generate(0, seed_samples=codes, return_proba_every=1,
                                 **({} if lc is None else
                                    dict(local_condition=lc[0, :len(codes) - 1])))
            torch.cuda.synchronize()
        sfx = '' if lc is None else '_lc'
        if path == 'single':
            assert 'wn_fastgen_run' + sfx in names, names
        elif path == 'steps':
            assert 'wn_fastgen_step' + sfx in names and net._gen['graphs'], names
        else:
            # the persistent launch ran, and did not hand over to the steps
            assert 'wn_fastgen_step' + sfx not in names, names
            assert 'fgp_sync' in net._gen and not net._gen_launch_failed.get('persist')
        assert np.array_equal(io.cpu().numpy(), codes), (tag, path)
        out[path] = p.cpu().numpy()
    return out


@pytest.mark.parametrize('gain', S.CASES['gen_mid'][2])
def test_fast_generation_32_channels(hip_lib, gain):
    """Single workgroup, step kernels under graph replay, persistent launch
    and the batched generator (B = 3) on a saturated 32-channel model: every
    step of a teacher-forced trace longer than the receptive field."""
    cfg = S.CASES['gen_mid'][0]
    net = _model(cfg, S.saturated_variables(cfg, gain))
    var = tree_to_numpy(net.variables)
    ref = _gen_ref('gen_mid', gain, var)
    got = _gen_paths(net, ('single', 'steps', 'persist'), ref[0], None, 'gen')
    for path, p in got.items():
        _check_probs('gen_%s-g%g' % (path, gain), p, ref)
    # the paths agree with each other as tests/test_gpu_model.py requires
    assert np.abs(got['steps'] - got['persist']).max() < 1e-6
    assert np.abs(got['single'] - got['steps']).max() < 1e-5
    refs = [_gen_ref('gen_mid', gain, var, s) for s in range(3)]
    with _spy(net) as (names, _):
        io, p = net.generate_batch(0, [11, 12, 13],
                                   seed_samples=np.stack([r[0] for r in refs]),
                                   return_proba_every=1)
        torch.cuda.synchronize()
    assert 'wn_fastgen_batch_step' in names, names
    p = p.cpu().numpy()
    for b in range(3):
        assert np.array_equal(io[b].cpu().numpy(), refs[b][0])
        _check_probs('gen_batch-g%g' % gain, p[b], refs[b])
    assert np.abs(p[0] - got['single']).max() < 1e-5


def test_fast_generation_wide(hip_lib):
    """wn_fastgen_run_wide on a saturated 64-channel model: the single
    workgroup and the cooperative launch."""
    cfg, _, gains, _ = S.CASES['gen_r64']
    net = _model(cfg, S.saturated_variables(cfg, gains[0]))
    assert hip_lib.wn_fastgen_wide_coop_bytes(net.L, net.CHn, net.S, net.Q) > 0
    var = tree_to_numpy(net.variables)
    ref = _gen_ref('gen_r64', gains[0], var)
    got = {}
    for coop in (False, True):
        net.fastgen_wide_coop = coop
        net.reset_generator()
        with _spy(net) as (names, _):
            io, p = net.generate(0, seed_samples=ref[0], return_proba_every=1)
            torch.cuda.synchronize()
        assert names.count('wn_fastgen_run_wide') == 1, names
        if coop:
            assert net._gen.get('coop') is not None
            assert not net._gen_launch_failed.get('coop')
        else:
            assert net._gen.get('coop') is None
        assert np.array_equal(io.cpu().numpy(), ref[0])
        got[coop] = p.cpu().numpy()
        _check_probs('gen_wide_%s-g%g' % ('coop' if coop else 'one_wg', gains[0]),
                     got[coop], ref)
    assert np.abs(got[True] - got[False]).max() < 1e-6


def test_fast_generation_local_conditioning(hip_lib):
    """The _lc entries (single workgroup, step kernels, persistent launch)
    with LC rows whose addend alone saturates gates."""
    cfg, _, gains, _ = S.CASES['gen_lc']
    net = _model(cfg, S.saturated_variables(cfg, gains[0]))
    var = tree_to_numpy(net.variables)
    ref = _gen_ref('gen_lc', gains[0], var)
    got = _gen_paths(net, ('single', 'steps', 'persist'), ref[0], ref[1], 'gen_lc')
    for path, p in got.items():
        _check_probs('gen_lc_%s-g%g' % (path, gains[0]), p, ref)
    assert np.abs(got['steps'] - got['persist']).max() < 1e-6
    assert np.abs(got['single'] - got['steps']).max() < 1e-5


# ------------------------------------------- softmax cross-entropy backward
def _xent_kernel(x, codes, lengths, Q, quirk):
    """wn_xent / wn_xent_masked alone -> (sum of the loss partials in float64,
    dlogits [B, T, ld] on a sentinel, the float32 factor it scaled by)."""
    from wavenet import _lib
    B, T, ld = x.shape
    dev = torch.device('cuda')
    xd = torch.as_tensor(x).to(dev).contiguous()
    qd = torch.as_tensor(codes).to(dev).contiguous()
    dl = torch.full((B, T, ld), -7.0, dtype=torch.float32, device=dev)
    parts = torch.zeros(int(_lib.load().wn_xent_partials(B * T)),
                        dtype=torch.float32, device=dev)
    if lengths is None:
        inv = np.float32(1.0) / np.float32(B * T)
        _lib.call('wn_xent', _lib.ptr(xd), ld, _lib.ptr(qd), _lib.ptr(dl),
                  _lib.ptr(parts), B, T, Q, int(quirk), _lib.stream())
    else:
        inv = np.float32(1.0) / np.float32(sum(lengths))
        mask = torch.from_numpy(np.concatenate(
            [np.asarray(lengths, np.int32),
             np.array([inv], np.float32).view(np.int32)])).to(dev)
        _lib.call('wn_xent_masked', _lib.ptr(xd), ld, _lib.ptr(qd),
                  _lib.ptr(mask), _lib.ptr(mask[B:]), _lib.ptr(dl),
                  _lib.ptr(parts), B, T, Q, int(quirk), _lib.stream())
    torch.cuda.synchronize()
    return float(parts.double().sum()), dl.cpu().numpy(), inv


@pytest.mark.parametrize('quirk', [1, 0], ids=['tf_quirk', 'exact'])
@pytest.mark.parametrize('B,T,Q,ld', [(3, 37, 256, 260), (2, 19, 64, 64)],
                         ids=['3x37_q256_ld260', '2x19_q64'])
def test_xent_backward_at_extreme_logits(hip_lib, B, T, Q, ld, quirk):
    """Loss and dlogits of wn_xent and wn_xent_masked on logits from
    uniform(-90, 90), with a row whose leader is 200 ahead (every other
    exponential is exactly 0) as the target, one where the target is such an
    underflowed entry, and a row of equal logits at 1e4."""
    rng = np.random.default_rng(B * T + Q)
    x = rng.uniform(-90, 90, (B, T, ld)).astype(np.float32)
    codes = rng.integers(0, Q, (B, T)).astype(np.int32)
    lead, other = 7, Q - 3
    for t in (3, 5):
        x[0, t, lead] = x[0, t, :Q].max() + 200.0
    codes[0, 4] = lead                  # row 3: the target leads
    codes[0, 6] = other                 # row 5: the target underflowed
    x[1, 2, :] = 1e4
    x[..., Q:] = 1e30                   # never read
    for lengths in (None, [T, 9, 20][:B]):
        tot64, g64, rows64 = S.xent(x[..., :Q], codes, lengths, 1.0, quirk, np.float64)
        assert rows64[0, 3] < 1e-30 and rows64[0, 5] > 199 and \
            abs(rows64[1, 2] - np.log(Q)) < 1e-9
        tot, dl, inv = _xent_kernel(x, codes, lengths, Q, quirk)
        tot64, g64, _ = S.xent(x[..., :Q], codes, lengths, inv, quirk, np.float64)
        tot32, g32, _ = S.xent(x[..., :Q], codes, lengths, inv, quirk, np.float32)
        assert tot32.dtype == np.float32 and g32.dtype == np.float32
        tag = 'xent_q%d%s%s' % (Q, '_masked' if lengths else '',
                                '_quirk' if quirk else '')
        assert np.isfinite(tot) and np.isfinite(dl).all()
        assert (dl[..., Q:] == -7.0).all()           # columns >= Q untouched
        e32 = abs(float(tot32) - tot64)
        _log(tag, 'loss', abs(tot - tot64), e32)
        assert abs(tot - tot64) <= 4.0 * e32, (tag, tot, tot64, e32)
        g = dl[..., :Q].astype(np.float64)
        e32 = np.abs(g32.astype(np.float64) - g64).max()
        _log(tag, 'dlogits', np.abs(g - g64).max(), e32)
        assert np.abs(g - g64).max() <= 4.0 * e32, (tag, np.abs(g - g64).max(), e32)
        # exact zeros: padding, and the label-less last row without the quirk
        if lengths is not None:
            for b, n in enumerate(lengths):
                assert not g[b, n:].any(), (tag, b)
        if not quirk:
            last = [T - 1] * B if lengths is None else [n - 1 for n in lengths]
            assert all(not g[b, last[b]].any() for b in range(B)), tag
        # the underflowed exponentials are exact zeros of the gradient
        off = np.ones(Q, bool)
        off[[lead, other]] = False
        assert not g[0, 5, off].any() and not g[0, 3, off].any(), tag
