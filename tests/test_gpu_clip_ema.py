"""Global-norm clipping and EMA weights on the GPU: the `_clip` updates against
the float64 restatement (tests/clip_ref.py), bitwise equality with the plain
optimizers when the clip is inactive, determinism of the norm partials, the
non-finite case, a wide bucket, two data-parallel ranks, and train.py /
generate.py end to end.  Every test prints the figures it asserts on."""
import copy
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import clip_ref
from util import (O, MID, ROOT, TINY, cfg_with, build_pair, flat_named,
                  model_kwargs, tree_to_numpy)

sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

KINDS = [('adam', 1e-3, 0.9), ('sgd', 0.02, 0.95), ('rmsprop', 1e-3, 0.9)]
# parameters (and the shadow, a convex combination of parameter iterates)
# against float64: the bound of test_gpu_model.py's optimizer trajectory test
PARAM_TOL = 2e-5
# the norm before clipping: float64 partials leave the final float32 rounding
# (6e-8) and the gradients' own error against float64
NORM_RTOL = 1e-5


def _audio(B=2, T=40, seed=2):
    return np.random.default_rng(seed).uniform(-1, 1, (B, T)).astype(
        np.float32)


def _shadow_tree(net, opt):
    return tree_to_numpy(net._views(opt._shadow))


def _max_diff(got_tree, ref_tree):
    return max(float(np.abs(a - b).max()) for (_, a), (_, b) in
               zip(flat_named(got_tree), flat_named(ref_tree)))


def _ref_tree(var, flat):
    return O.unpack_into(copy.deepcopy(var), flat)


def _run_vs_ref(cfg, audio, kind, lr, mom, clip_norm, decay, steps):
    """`steps` steps of the HIP optimizer and of clip_ref on the same
    weights; returns (max parameter error, max shadow error, max relative
    norm error, the float64 norms)."""
    from wavenet import optimizer_factory
    net, var = build_pair(cfg)
    opt = optimizer_factory[kind](learning_rate=lr, momentum=mom,
                                  clip_norm=clip_norm, ema_decay=decay)
    ref = clip_ref.ClipEMAOptimizer(kind, lr, mom, clip_norm, decay)
    nerr, norms = 0.0, []
    for _ in range(steps):
        _, g = O.loss_and_grads(cfg, var, audio, dtype=np.float64)
        O.unpack_into(var, ref.apply(O.pack(var), O.pack(g)))
        opt.minimize(net.loss(audio))
        got = float(opt.last_grad_norm)
        nerr = max(nerr, abs(got - ref.last_norm) / ref.last_norm)
        norms.append(ref.last_norm)
    perr = _max_diff(tree_to_numpy(net.variables), var)
    serr = _max_diff(_shadow_tree(net, opt), _ref_tree(var, ref.shadow))
    return perr, serr, nerr, norms


@pytest.mark.parametrize('kind,lr,mom', KINDS)
def test_parity_with_float64(hip_lib, kind, lr, mom):
    """Three steps on TINY (the model, audio and rates of
    test_gpu_model.py::test_optimizer_trajectory_vs_oracle) with clip_norm =
    half (active) and twice (inactive at step 1) the float64 reference's own
    step-1 norm, EMA decay 0.9: parameters and shadow within 2e-5 of
    clip_ref, last_grad_norm within a relative 1e-5 of the float64 norm."""
    cfg = cfg_with(TINY, batch_size=2)
    audio = _audio()
    _, var = build_pair(cfg)
    _, g = O.loss_and_grads(cfg, var, audio, dtype=np.float64)
    norm1 = clip_ref.global_norm(O.pack(g))
    assert norm1 > 0
    for mult in (0.5, 2.0):
        perr, serr, nerr, norms = _run_vs_ref(cfg, audio, kind, lr, mom,
                                              mult * norm1, 0.9, 3)
        print('parity %s clip %.1f x norm1 (%.4f): params %.3e shadow %.3e '
              'norm rel %.3e, norms %s' % (kind, mult, norm1, perr, serr, nerr,
                                           ['%.4f' % n for n in norms]))
        assert abs(norms[0] - norm1) < 1e-12
        assert perr < PARAM_TOL and serr < PARAM_TOL
        assert nerr < NORM_RTOL


def _five_steps(kind, lr, mom, **kw):
    from wavenet import optimizer_factory
    cfg = cfg_with(TINY, batch_size=2)
    net, _ = build_pair(cfg)
    opt = optimizer_factory[kind](learning_rate=lr, momentum=mom, **kw)
    for s in range(5):
        opt.minimize(net.loss(_audio(seed=10 + s)))
    torch.cuda.synchronize()
    return net, opt


@pytest.mark.parametrize('kind,lr,mom', KINDS)
def test_inactive_clip_is_bitwise_the_plain_optimizer(hip_lib, kind, lr, mom):
    """clip_norm = 1e30 never clips: bucket, slots and parameters after five
    steps equal the plain optimizer's bit for bit; ema_decay alone leaves the
    parameters bitwise unchanged as well (and moves the shadow)."""
    net0, opt0 = _five_steps(kind, lr, mom)
    net1, opt1 = _five_steps(kind, lr, mom, clip_norm=1e30)
    assert torch.equal(net0.grads, net1.grads)
    assert torch.equal(net0.params, net1.params)
    assert len(opt0._slots) == len(opt1._slots)
    for a, b in zip(opt0._slots, opt1._slots):
        assert torch.equal(a, b)
    assert 0 < float(opt1.last_grad_norm) < 1e30
    net2, opt2 = _five_steps(kind, lr, mom, ema_decay=0.9)
    assert torch.equal(net0.params, net2.params)
    for a, b in zip(opt0._slots, opt2._slots):
        assert torch.equal(a, b)
    assert opt2.last_grad_norm is None
    assert not torch.equal(opt2._shadow, net2.params)
    net3, opt3 = _five_steps(kind, lr, mom, clip_norm=1e30, ema_decay=0.9)
    assert torch.equal(net0.params, net3.params)
    assert torch.equal(opt2._shadow, opt3._shadow)
    # an active clip does change the step
    net4, _ = _five_steps(kind, lr, mom, clip_norm=1e-3)
    assert not torch.equal(net0.params, net4.params)


def test_active_clip_step_is_deterministic(hip_lib):
    """Two runs of the same active-clip steps give identical bits."""
    runs = [_five_steps('adam', 1e-3, 0.9, clip_norm=0.01, ema_decay=0.99)
            for _ in range(2)]
    (n0, o0), (n1, o1) = runs
    assert float(o0.last_grad_norm) > 0.01          # the clip is active
    assert torch.equal(n0.params, n1.params)
    assert torch.equal(o0._shadow, o1._shadow)
    assert torch.equal(o0.last_grad_norm, o1.last_grad_norm)
    assert torch.equal(o0._gn_parts, o1._gn_parts)
    for a, b in zip(o0._slots, o1._slots):
        assert torch.equal(a, b)


def _partials(bucket):
    from wavenet import _lib
    parts = torch.zeros(_lib.load().wn_grad_norm_partials_count(),
                        dtype=torch.float64, device=bucket.device)
    _lib.call('wn_grad_norm_partials', _lib.ptr(bucket), bucket.numel(),
              _lib.ptr(parts), _lib.stream())
    torch.cuda.synchronize()
    return parts.cpu().numpy()


def test_partials_depend_on_the_bucket_alone(hip_lib):
    """The partials of one bucket are the same bits whatever launches the
    model around it runs (stack_variant, batch shape), each is the float64
    sum of squares of its contiguous range, and odd sizes (ranges that end
    off a 16-byte group, empty ranges) are covered."""
    from wavenet import WaveNetModel, _lib
    cfg = cfg_with(MID, batch_size=2)
    net, _ = build_pair(cfg)
    net.loss(_audio(2, 300))
    bucket = net.grads.clone()
    want = _partials(bucket)
    P = want.size
    n = bucket.numel()
    per = -(-n // (4 * P)) * 4
    g = bucket.cpu().numpy().astype(np.float64)
    ref = np.array([np.sum(g[k * per:(k + 1) * per] ** 2) for k in range(P)])
    print('partials: n %d, per %d, max rel err vs float64 %.3e' % (
        n, per, np.abs(want - ref).max() / ref.max()))
    assert np.abs(want - ref).max() <= 1e-14 * ref.max()
    for variant, B, T in ((_lib.stack_variant(rows=16), 1, 500),
                          (_lib.stack_variant(rows=32), 3, 200),
                          (0, 4, 64)):
        other = WaveNetModel(**model_kwargs(cfg_with(MID, batch_size=B)))
        other.stack_variant = variant
        other.loss(_audio(B, T))
        assert other.grads.numel() == n
        other.grads.copy_(bucket)
        assert np.array_equal(_partials(other.grads), want), (variant, B, T)
    rng = np.random.default_rng(5)
    for m in (1, 3, 4, 5, 1023, 1024, 1029, 70001):
        x = torch.from_numpy(rng.standard_normal(m).astype(np.float32)).cuda()
        got = _partials(x)
        perm = -(-m // (4 * P)) * 4
        xr = x.cpu().numpy().astype(np.float64)
        refm = np.array([np.sum(xr[k * perm:(k + 1) * perm] ** 2)
                         for k in range(P)])
        assert np.abs(got - refm).max() <= 1e-14 * max(refm.max(), 1e-300), m
        assert abs(got.sum() - np.sum(xr ** 2)) <= 1e-13 * np.sum(xr ** 2)


@pytest.mark.parametrize('kind,lr,mom', KINDS)
def test_non_finite_bucket_gives_nan_parameters(hip_lib, kind, lr, mom):
    """One inf in the bucket: a non-finite norm, a NaN factor, NaN
    parameters -- no silent skip."""
    from wavenet import optimizer_factory
    cfg = cfg_with(TINY, batch_size=2)
    net, _ = build_pair(cfg)
    opt = optimizer_factory[kind](learning_rate=lr, momentum=mom,
                                  clip_norm=1.0, ema_decay=0.9)
    loss = net.loss(_audio())
    net.grads[net.grads.numel() // 3] = torch.tensor(float('inf'))
    opt.minimize(loss)
    torch.cuda.synchronize()
    assert not np.isfinite(float(opt.last_grad_norm))
    for n, v in net.named_variables():
        assert bool(torch.isnan(v).all()), n
    assert bool(torch.isnan(net.params).all())


def test_wide_bucket_clipped_step(hip_lib):
    """One clipped step of a 64-channel model (two channel blocks per layer,
    another bucket layout) against clip_ref, clip_norm = half the float64
    norm."""
    cfg = cfg_with(MID, batch_size=2, residual_channels=64,
                   dilation_channels=64, skip_channels=32)
    audio = _audio(2, 150, seed=4)
    _, var = build_pair(cfg)
    _, g = O.loss_and_grads(cfg, var, audio, dtype=np.float64)
    norm1 = clip_ref.global_norm(O.pack(g))
    perr, serr, nerr, _ = _run_vs_ref(cfg, audio, 'adam', 1e-3, 0.9,
                                      0.5 * norm1, 0.9, 1)
    print('wide: norm %.4f, params %.3e shadow %.3e norm rel %.3e'
          % (norm1, perr, serr, nerr))
    assert perr < PARAM_TOL and serr < PARAM_TOL and nerr < NORM_RTOL


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks_clip_same_bits_and_float64_step(hip_lib, tmp_path):
    """Two ranks on this GPU (gloo), different shards of one batch of four
    clips, active clip and EMA, two momentum steps.  Both ranks derive the
    factor from the same all-reduced bucket: parameters, shadow and norms are
    bitwise equal across the ranks, and within 1e-6 (the bound of
    test_gpu_parallel.py) of clip_ref's float64 steps on the global batch.
    (Momentum updates: a parameter's error is lr times its gradient's.  Adam
    divides by sqrt(v) + 1e-4, which multiplies a small gradient's error by
    up to 10 in the first steps and so belongs with the 2e-5 of the parity
    test above, not with this bound.)"""
    import clip_dp_worker
    from wavenet import WaveNetModel
    spec = dict(B=4, T=300, steps=2, opt='sgd', lr=0.02, ema_decay=0.9)
    cfg = cfg_with(MID, batch_size=4)
    var = O.create_variables(cfg, seed=0, dtype=np.float64, bias_scale=0.1)
    audio = clip_dp_worker.batch(spec)
    _, g = O.loss_and_grads(cfg, var, audio[0], dtype=np.float64)
    spec['clip_norm'] = 0.5 * clip_ref.global_norm(O.pack(g))
    ref = clip_ref.ClipEMAOptimizer('sgd', 0.02, 0.9, spec['clip_norm'], 0.9)
    ref_norms = []
    for s in range(spec['steps']):
        _, g = O.loss_and_grads(cfg, var, audio[s], dtype=np.float64)
        O.unpack_into(var, ref.apply(O.pack(var), O.pack(g)))
        ref_norms.append(ref.last_norm)
    assert ref_norms[0] > spec['clip_norm']
    spec['out'] = str(tmp_path / 'rank%d.npz')
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE='2',
                   MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY='0', WN_SHARE_GPU='1',
                   WN_DIST_BACKEND='gloo', WN_DIST_TIMEOUT='120')
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(HERE, 'clip_dp_worker.py'),
             json.dumps(spec)], env=env, stdout=subprocess.PIPE,
            stderr=subprocess.STDOUT))
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            p.kill()
            o, _ = p.communicate()
        outs.append(o.decode(errors='replace'))
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    a, b = (np.load(spec['out'] % r) for r in range(2))
    for k in ('params', 'shadow', 'norms'):
        assert np.array_equal(a[k], b[k]), k
    cpu = WaveNetModel(device='cpu', **model_kwargs(cfg))
    perr = _max_diff(tree_to_numpy(cpu._views(torch.from_numpy(a['params']))),
                     var)
    serr = _max_diff(tree_to_numpy(cpu._views(torch.from_numpy(a['shadow']))),
                     _ref_tree(var, ref.shadow))
    nerr = np.abs(a['norms'] / np.asarray(ref_norms) - 1).max()
    print('dp: params %.3e shadow %.3e norm rel %.3e, norms %s clip %.4f'
          % (perr, serr, nerr, ref_norms, spec['clip_norm']))
    assert perr <= 1e-6 and serr <= 1e-6
    assert nerr < NORM_RTOL


SMALL = {"filter_width": 2, "sample_rate": 16000,
         "dilations": [1, 2, 4, 8, 16, 32, 1, 2, 4, 8, 16, 32],
         "residual_channels": 32, "dilation_channels": 32,
         "quantization_channels": 256, "skip_channels": 64,
         "use_biases": True, "scalar_input": False,
         "initial_filter_width": 32, "residual_postproc": False}


def test_train_py_clip_ema_checkpoint_resume_generate(hip_lib, tmp_path,
                                                      capsys):
    """train.py --synthetic --clip_norm --ema_decay trains, logs the norm
    before clipping one step late beside the loss and checkpoints optimizer
    and EMA weights; a restart restores Adam's step count and slots;
    generate.py --use_ema true runs from the checkpoint."""
    import generate
    import train
    pj = str(tmp_path / 'params.json')
    json.dump(SMALL, open(pj, 'w'))
    logdir = str(tmp_path / 'run')
    common = ['--synthetic', '--sample_size', '3000', '--batch_size', '2',
              '--wavenet_params', pj, '--logdir', logdir,
              '--checkpoint_every', '2', '--learning_rate', '0.002',
              '--clip_norm', '0.5', '--ema_decay', '0.9']
    assert train.main(common + ['--num_steps', '5']) == 0
    out = capsys.readouterr().out
    assert 'step 0 - loss = ' in out and ', grad norm = ' in out
    ev = [json.loads(l) for l in open(os.path.join(logdir, 'events.jsonl'))]
    assert [e['step'] for e in ev] == [0, 1, 2, 3, 4]
    assert all(np.isfinite(e['grad_norm']) and e['grad_norm'] > 0 for e in ev)
    assert ev[-1]['loss'] < ev[0]['loss']
    ck4 = torch.load(os.path.join(logdir, 'model.ckpt-4'), map_location='cpu')
    assert ck4['optimizer']['step'] == 5 and ck4['optimizer']['kind'] == \
        'AdamOptimizer'
    assert list(ck4['ema_variables']) == list(ck4['variables'])
    k = 'wavenet/postprocessing/postprocess2'
    assert not torch.equal(ck4['ema_variables'][k], ck4['variables'][k])
    assert float(ck4['optimizer']['slots'][1].abs().max()) > 0
    # restart: two more steps, Adam's count goes on from 5
    assert train.main(common + ['--num_steps', '7']) == 0
    out = capsys.readouterr().out
    assert 'Global step was: 4' in out and 'step 5 - loss' in out
    ck = os.path.join(logdir, 'model.ckpt-6')
    ck6 = torch.load(ck, map_location='cpu')
    assert ck6['optimizer']['step'] == 7
    # without the flags: none of the new output, no 'ema_variables'
    plain = str(tmp_path / 'plain')
    assert train.main(['--synthetic', '--sample_size', '3000', '--batch_size',
                       '2', '--wavenet_params', pj, '--logdir', plain,
                       '--num_steps', '2']) == 0
    out = capsys.readouterr().out
    assert 'grad norm' not in out
    pk = torch.load(train.latest_checkpoint(plain), map_location='cpu')
    assert 'ema_variables' not in pk and pk['optimizer']['step'] == 2
    assert all('grad_norm' not in json.loads(l) for l in
               open(os.path.join(plain, 'events.jsonl')))
    # generation from the EMA weights and from the raw ones differ
    codes = []
    for flag in ('true', 'false'):
        gen = str(tmp_path / ('gen_' + flag))
        assert generate.main([ck, '--samples', '200', '--wavenet_params', pj,
                              '--use_ema', flag, '--logdir', gen]) == 0
        run = os.path.join(gen, 'generate')
        codes.append(np.load(os.path.join(run, os.listdir(run)[0],
                                          'generated_codes.npy')))
    capsys.readouterr()
    assert codes[0].shape == codes[1].shape == (201,)
    assert generate.main([train.latest_checkpoint(plain), '--samples', '10',
                          '--wavenet_params', pj, '--use_ema', 'true']) == 1
    assert 'ema_variables' in capsys.readouterr().out


@pytest.mark.parametrize('kind,lr,mom', KINDS)
def test_resumed_step_is_bitwise_the_uninterrupted_one(hip_lib, tmp_path,
                                                       kind, lr, mom):
    """Three steps, train.save, train.load into a new model and optimizer,
    one more step: parameters, slots and shadow equal the fourth step of the
    uninterrupted run bit for bit (step count, hence Adam's bias correction,
    slots and shadow all restored).  In process, on the same batches: a
    restarted train.py --synthetic draws its clips anew, so its steps cannot
    be compared with an uninterrupted run's."""
    import train
    from wavenet import optimizer_factory
    cfg = cfg_with(TINY, batch_size=2)
    kw = dict(learning_rate=lr, momentum=mom, clip_norm=0.01, ema_decay=0.9)

    def steps(net, opt, lo, hi):
        for s in range(lo, hi):
            opt.minimize(net.loss(_audio(seed=30 + s)))
        torch.cuda.synchronize()

    net_a, _ = build_pair(cfg)
    opt_a = optimizer_factory[kind](**kw)
    steps(net_a, opt_a, 0, 4)
    net_b, _ = build_pair(cfg)
    opt_b = optimizer_factory[kind](**kw)
    steps(net_b, opt_b, 0, 3)
    train.save(net_b, str(tmp_path), 2, opt_b)
    net_c, _ = build_pair(cfg, seed=7)
    opt_c = optimizer_factory[kind](**kw)
    assert train.load(net_c, str(tmp_path), opt_c) == 2
    steps(net_c, opt_c, 3, 4)
    assert opt_c._step == 4
    assert torch.equal(net_c.params, net_a.params)
    assert torch.equal(opt_c._shadow, opt_a._shadow)
    for a, b in zip(opt_a._slots, opt_c._slots):
        assert torch.equal(a, b)
    assert torch.equal(opt_c.last_grad_norm, opt_a.last_grad_norm)
    if kind == 'adam':
        # without the optimizer entry the restart is another step
        net_d, _ = build_pair(cfg, seed=7)
        opt_d = optimizer_factory[kind](**kw)
        assert train.load(net_d, str(tmp_path)) == 2
        steps(net_d, opt_d, 3, 4)
        assert not torch.equal(net_d.params, net_a.params)


# ---- the entry points themselves: the L2 arm and the EMA epilogue ----------
def _abi_step(kind, lr, mom, step, clip, p, g, slots, l2=0.0, mask=None,
              ema=None, decay=0.0):
    """One update through wn_X (clip False) or wn_X_clip with partials = None
    (the clip inactive), on device tensors, in place."""
    import math
    from wavenet import _lib
    stem, rule = {
        'adam': ('adam', (lr * math.sqrt(1.0 - 0.999 ** step) /
                          (1.0 - 0.9 ** step), 0.9, 0.999, 1e-4)),
        'sgd': ('momentum', (lr, mom)),
        'rmsprop': ('rmsprop', (lr, 0.9, mom, 1e-5))}[kind]
    tail = (None, 0, 0.0, _lib.ptr(ema), decay, None) if clip else ()
    _lib.call('wn_' + stem + ('_clip' if clip else ''), _lib.ptr(p),
              _lib.ptr(g), *[_lib.ptr(s) for s in slots], p.numel(), *rule,
              1.0, l2, _lib.ptr(mask), *(tail + (_lib.stream(),)))


def _abi_inputs(kind, n, seed):
    rng = np.random.default_rng(seed)
    w = rng.uniform(-1, 1, n).astype(np.float32)
    gs = [(0.1 * rng.uniform(-1, 1, n)).astype(np.float32) for _ in range(2)]
    mask = (rng.random(n) < 0.5).astype(np.float32)
    slots = [np.ones(n, np.float32), np.zeros(n, np.float32)] \
        if kind == 'rmsprop' else \
        [np.zeros(n, np.float32) for _ in range(2 if kind == 'adam' else 1)]
    return w, gs, mask, slots


def _dev(a):
    return torch.as_tensor(a).to('cuda').clone()


# 1031: no multiple of 4 or 256 (the loop's ragged end); the other is past
# the 2048-workgroup cap of the launch (a second trip of the grid-stride loop)
L2_NS = [1031, 2048 * 256 + 1031]


@pytest.mark.parametrize('n', L2_NS)
@pytest.mark.parametrize('kind,lr,mom', KINDS)
def test_l2_arm_of_both_entry_points(hip_lib, kind, lr, mom, n):
    """l2 = 0.01 with a mask of zeros and ones, two steps: wn_X and wn_X_clip
    (partials = None, ema = None) leave the same bits in parameters and slots,
    and both are within PARAM_TOL of the float64 rule (tests/clip_ref.py with
    its l2 * w * mask term)."""
    w, gs, mask, slots = _abi_inputs(kind, n, n + len(kind))
    runs = []
    for clip in (False, True):
        p, sl, mk = _dev(w), [_dev(s) for s in slots], _dev(mask)
        for step, g in enumerate(gs, 1):
            _abi_step(kind, lr, mom, step, clip, p, _dev(g), sl, 0.01, mk)
        torch.cuda.synchronize()
        runs.append([p] + sl)
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    ref = clip_ref.ClipEMAOptimizer(kind, lr, mom)
    w64 = w.astype(np.float64)
    for g in gs:
        w64 = ref.apply(w64, g, l2=0.01, l2_mask=mask)
    assert mask.min() == 0.0 and mask.max() == 1.0
    errs = [float(np.abs(a.cpu().numpy() - b).max())
            for a, b in zip(runs[0], [w64] + ref.opt.slots)]
    print('l2 arm %s n %d: parameter and slot errors %s (bar %.0e)'
          % (kind, n, ['%.3e' % e for e in errs], PARAM_TOL))
    assert max(errs) < PARAM_TOL
    # the term acts, and only where the mask is one
    q, sq = _dev(w), [_dev(s) for s in slots]
    _abi_step(kind, lr, mom, 1, False, q, _dev(gs[0]), sq)
    _abi_step(kind, lr, mom, 2, False, q, _dev(gs[1]), sq)
    same = (q == runs[0][0]).cpu().numpy()
    assert same[mask == 0].all() and not same[mask == 1].all()


@pytest.mark.parametrize('kind,lr,mom', KINDS)
def test_ema_epilogue_with_the_clip_inactive(hip_lib, kind, lr, mom):
    """wn_X_clip with partials = None and a shadow, n = 1031: the parameters
    are the plain entry point's, the shadow is  s - (1 - decay) (s - p_new)
    evaluated in float32 from the returned p_new, bit for bit."""
    n, decay = 1031, 0.9
    w, gs, _, slots = _abi_inputs(kind, n, 77)
    s0 = np.random.default_rng(78).uniform(-1, 1, n).astype(np.float32)
    p0, sl0 = _dev(w), [_dev(s) for s in slots]
    _abi_step(kind, lr, mom, 1, False, p0, _dev(gs[0]), sl0)
    p1, sl1, ema = _dev(w), [_dev(s) for s in slots], _dev(s0)
    _abi_step(kind, lr, mom, 1, True, p1, _dev(gs[0]), sl1, ema=ema,
              decay=decay)
    torch.cuda.synchronize()
    assert torch.equal(p0, p1)
    for a, b in zip(sl0, sl1):
        assert torch.equal(a, b)
    pn = p1.cpu().numpy()
    keep = np.float32(1.0) - np.float32(decay)
    want = s0 - keep * (s0 - pn)
    assert want.dtype == np.float32
    assert np.array_equal(ema.cpu().numpy().view(np.int32),
                          want.view(np.int32))
    assert not np.array_equal(want, s0)
