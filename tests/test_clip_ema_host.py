"""Global-norm clipping and EMA weights without a GPU: keyword validation
before the library or a device is touched, the factory's call compatibility,
the order of minimize's calls, argument validation of the new entry points,
optimizer / checkpoint round trips on device='cpu' models, generate.py's
--use_ema error path, and the float64 restatement (tests/clip_ref.py) against
hand-computed identities."""
import ctypes
import inspect
import math
import sys

import numpy as np
import pytest
import torch

import clip_ref
from util import ROOT

sys.path.insert(0, ROOT)

KINDS = ['adam', 'sgd', 'rmsprop']


def _net(**kw):
    from wavenet import WaveNetModel
    args = dict(batch_size=2, dilations=[1, 2, 4, 8], filter_width=2,
                residual_channels=32, dilation_channels=32, skip_channels=64,
                quantization_channels=256, use_biases=True, device='cpu')
    args.update(kw)
    return WaveNetModel(**args)


# ---------------------------------------------------------------- keywords
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('kw', [
    dict(clip_norm=0.0), dict(clip_norm=-1.0), dict(clip_norm=float('inf')),
    dict(clip_norm=float('nan')), dict(clip_norm='1'), dict(clip_norm=True),
    dict(clip_norm=1e39),
    dict(ema_decay=1.0), dict(ema_decay=-0.1), dict(ema_decay=float('nan')),
    dict(ema_decay=1.5), dict(ema_decay='0.9'), dict(ema_decay=1 - 1e-12)])
def test_bad_keywords_raise_before_library_or_device(kind, kw, monkeypatch):
    from wavenet import _lib, optimizer_factory
    monkeypatch.setattr(_lib, 'load', lambda: pytest.fail('library touched'))
    monkeypatch.setattr(_lib, 'require_gpu',
                        lambda: pytest.fail('device touched'))
    with pytest.raises(ValueError, match=list(kw)[0]):
        optimizer_factory[kind](learning_rate=1e-3, momentum=0.9, **kw)


@pytest.mark.parametrize('kind', KINDS)
def test_good_keywords_and_keyword_only(kind, monkeypatch):
    from wavenet import _lib, ops, optimizer_factory
    monkeypatch.setattr(_lib, 'load', lambda: pytest.fail('library touched'))
    monkeypatch.setattr(_lib, 'require_gpu',
                        lambda: pytest.fail('device touched'))
    o = optimizer_factory[kind](learning_rate=1e-3, momentum=0.9,
                                clip_norm=5, ema_decay=0.0)
    assert o.clip_norm == 5.0 and o.ema_decay == 0.0
    assert o.last_grad_norm is None
    o = optimizer_factory[kind](learning_rate=1e-3, momentum=0.9,
                                ema_decay=0.9999)
    assert o.clip_norm is None and o.ema_decay == 0.9999
    for fn in (optimizer_factory[kind], type(o).__init__):
        for name in ('clip_norm', 'ema_decay'):
            p = inspect.signature(fn).parameters[name]
            assert p.kind == p.KEYWORD_ONLY and p.default is None
    with pytest.raises(TypeError):
        optimizer_factory[kind](1e-3, 0.9, 5.0)
    assert set(ops.optimizer_factory) == {'adam', 'sgd', 'rmsprop'}


@pytest.mark.parametrize('kind', KINDS)
def test_factory_stays_call_compatible(kind):
    from wavenet import optimizer_factory
    o = optimizer_factory[kind](learning_rate=1e-3, momentum=0.9)
    assert o.clip_norm is None and o.ema_decay is None
    o = optimizer_factory[kind](1e-3, 0.9)
    assert o.lr == 1e-3 and o.last_grad_norm is None


# -------------------------------------------------------------- call order
OLD = {'adam': 'wn_adam', 'sgd': 'wn_momentum', 'rmsprop': 'wn_rmsprop'}


def _recorded_minimize(monkeypatch, kind, **kw):
    from wavenet import _lib, optimizer_factory, parallel
    net = _net()
    log = []

    class FakeLib(object):
        def wn_grad_norm_partials_count(self):
            return 256
    monkeypatch.setattr(_lib, 'load', lambda: FakeLib())
    monkeypatch.setattr(_lib, 'stream', lambda: 0)
    monkeypatch.setattr(_lib, 'call', lambda name, *a: log.append((name, a)))
    monkeypatch.setattr(parallel, 'allreduce_gradients',
                        lambda m: log.append(('allreduce', (m,))) or 0.5)
    opt = optimizer_factory[kind](learning_rate=1e-3, momentum=0.9, **kw)
    loss = torch.zeros(())
    loss._wn_model, loss._wn_has_grads = net, True
    assert opt.minimize(loss) is loss
    return net, opt, log


@pytest.mark.parametrize('kind', KINDS)
def test_call_order_allreduce_partials_update(hip_lib, monkeypatch, kind):
    net, opt, log = _recorded_minimize(monkeypatch, kind, clip_norm=2.0,
                                       ema_decay=0.99)
    assert [n for n, _ in log] == ['allreduce', 'wn_grad_norm_partials',
                                   OLD[kind] + '_clip']
    parts = log[1][1]
    assert parts[0] == net.grads.data_ptr() and parts[1] == net.grads.numel()
    a = log[2][1]
    # ..., partials, nparts, clip_norm, ema, ema_decay, norm_out, stream
    assert a[-7] == parts[2] and a[-6] == 256 and a[-5] == 2.0
    assert a[-4] == opt._shadow.data_ptr() and a[-3] == 0.99
    assert a[-2] == opt.last_grad_norm.data_ptr()
    assert a[0] == net.params.data_ptr() and a[1] == net.grads.data_ptr()
    # the all-reduce's 1 / N is the update's grad_scale
    assert 0.5 in a
    # the shadow starts as a copy of the parameters
    assert opt._shadow is not net.params
    assert torch.equal(opt._shadow, net.params)
    assert opt.last_grad_norm.dtype == torch.float32
    assert opt.last_grad_norm.shape == ()


@pytest.mark.parametrize('kind', KINDS)
def test_ema_alone_launches_no_partials(hip_lib, monkeypatch, kind):
    net, opt, log = _recorded_minimize(monkeypatch, kind, ema_decay=0.5)
    assert [n for n, _ in log] == ['allreduce', OLD[kind] + '_clip']
    a = log[1][1]
    assert a[-7] is None and a[-6] == 0 and a[-2] is None
    assert a[-4] == opt._shadow.data_ptr()
    assert opt.last_grad_norm is None


@pytest.mark.parametrize('kind', KINDS)
def test_without_keywords_only_the_old_entry_point(hip_lib, monkeypatch, kind):
    net, opt, log = _recorded_minimize(monkeypatch, kind)
    assert [n for n, _ in log] == ['allreduce', OLD[kind]]
    assert opt._shadow is None and opt.last_grad_norm is None
    want = {'adam': 13, 'sgd': 10, 'rmsprop': 13}[kind]
    assert len(log[1][1]) == want          # the signature of before


# ------------------------------------------------------ library validation
def test_new_entry_points_validate_without_gpu(hip_lib):
    lib = hip_lib
    assert lib.wn_grad_norm_partials_count() == 256
    buf = (ctypes.c_double * 512)()
    a = ctypes.addressof(buf)
    assert a % 16 == 0 or (a + 8) % 16 == 0
    a += a % 16                                   # 16-byte aligned
    assert lib.wn_grad_norm_partials(None, 8, a, None) == -5
    assert lib.wn_grad_norm_partials(a, 8, None, None) == -5
    assert lib.wn_grad_norm_partials(a, 0, a, None) == -1
    assert lib.wn_grad_norm_partials(a + 4, 8, a, None) == -3
    assert lib.wn_grad_norm_partials(a, 8, a + 4, None) == -3

    def adam(p=a, parts=a, nparts=256, clip=1.0, ema=a, decay=0.5, out=a):
        return lib.wn_adam_clip(p, a, a, a, 8, 1e-3, 0.9, 0.999, 1e-4, 1.0,
                                0.0, None, parts, nparts, clip, ema, decay,
                                out, None)

    def sgd(p=a, parts=a, nparts=256, clip=1.0, ema=a, decay=0.5, out=a):
        return lib.wn_momentum_clip(p, a, a, 8, 1e-3, 0.9, 1.0, 0.0, None,
                                    parts, nparts, clip, ema, decay, out, None)

    def rms(p=a, parts=a, nparts=256, clip=1.0, ema=a, decay=0.5, out=a):
        return lib.wn_rmsprop_clip(p, a, a, a, 8, 1e-3, 0.9, 0.9, 1e-5, 1.0,
                                   0.0, None, parts, nparts, clip, ema, decay,
                                   out, None)

    for fn in (adam, sgd, rms):
        assert fn(p=None) == -5
        assert fn(nparts=255) == -1 and fn(nparts=0) == -1
        assert fn(clip=0.0) == -1 and fn(clip=float('inf')) == -1
        assert fn(clip=float('nan')) == -1 and fn(clip=-2.0) == -1
        assert fn(decay=1.0) == -1 and fn(decay=-0.5) == -1
        assert fn(decay=float('nan')) == -1
        assert fn(parts=a + 4) == -3
        assert fn(ema=a + 2) == -3
        assert fn(out=a + 2) == -3
    assert lib.wn_adam_clip(a, a, a, a, 0, 1e-3, 0.9, 0.999, 1e-4, 1.0, 0.0,
                            None, None, 0, 0.0, None, 0.0, None, None) == -1


# ------------------------------------------------------------- state dicts
@pytest.mark.parametrize('kind', KINDS)
def test_state_dict_round_trip(hip_lib, kind):
    from wavenet import optimizer_factory
    net = _net()
    a = optimizer_factory[kind](learning_rate=1e-3, momentum=0.9,
                                clip_norm=1.0, ema_decay=0.9)
    a.init_state(net)
    g = torch.Generator().manual_seed(1)
    for s in a._slots:
        s.copy_(torch.rand(s.shape, generator=g))
    assert torch.equal(a._shadow, net.params)
    a._shadow.copy_(torch.rand(a._shadow.shape, generator=g))
    a._step = 17
    sd = a.state_dict()
    assert sd['step'] == 17 and len(sd['slots']) == len(a._slots)
    assert all(t.device.type == 'cpu' for t in sd['slots'] + [sd['shadow']])
    b = optimizer_factory[kind](learning_rate=1e-3, momentum=0.9,
                                clip_norm=1.0, ema_decay=0.9)
    b.load_state_dict(sd, net)
    assert b._step == 17
    for x, y in zip(a._slots, b._slots):
        assert torch.equal(x, y) and x is not y
    assert torch.equal(a._shadow, b._shadow)
    # the shadow under the model's own keys, loadable by the model
    es = b.ema_state_dict(net)
    assert list(es) == list(net.state_dict())
    other = _net(seed=9)
    other.load_state_dict(es)
    for (n, v), (_, w) in zip(other.named_variables(), net.named_variables(
            net._views(b._shadow))):
        assert torch.equal(v, w), n
    # a state without shadow: the shadow starts from the parameters
    plain = optimizer_factory[kind](learning_rate=1e-3, momentum=0.9)
    plain.init_state(net)
    sd0 = plain.state_dict()
    assert sd0['shadow'] is None
    c = optimizer_factory[kind](learning_rate=1e-3, momentum=0.9,
                                ema_decay=0.5)
    c.load_state_dict(sd0, net)
    c.init_state(net)
    assert torch.equal(c._shadow, net.params)
    # wrong kind / wrong model
    wrong = optimizer_factory['sgd' if kind != 'sgd' else 'adam'](
        learning_rate=1e-3, momentum=0.9)
    with pytest.raises(ValueError, match='cannot be loaded'):
        wrong.load_state_dict(sd, net)
    with pytest.raises(ValueError, match='floats'):
        b.load_state_dict(sd, _net(dilations=[1, 2]))
    with pytest.raises(ValueError, match='ema_decay'):
        plain.ema_state_dict(net)


def test_train_save_load_round_trip(hip_lib, tmp_path, capsys):
    import train
    from wavenet import optimizer_factory
    net = _net(seed=2)
    opt = optimizer_factory['adam'](learning_rate=1e-3, momentum=0.9,
                                    clip_norm=3.0, ema_decay=0.75)
    opt.init_state(net)
    g = torch.Generator().manual_seed(3)
    for s in opt._slots + [opt._shadow]:
        s.copy_(torch.rand(s.shape, generator=g))
    opt._step = 5
    logdir = str(tmp_path / 'run')
    train.save(net, logdir, 4, opt)
    ck = torch.load(train.latest_checkpoint(logdir), map_location='cpu')
    assert set(ck) == {'variables', 'step', 'optimizer', 'ema_variables'}
    assert list(ck['ema_variables']) == list(ck['variables'])
    net2 = _net(seed=8)
    opt2 = optimizer_factory['adam'](learning_rate=1e-3, momentum=0.9,
                                     clip_norm=3.0, ema_decay=0.75)
    assert train.load(net2, logdir, opt2) == 4
    assert torch.equal(net2.params, net.params)
    assert opt2._step == 5
    for x, y in zip(opt._slots + [opt._shadow], opt2._slots + [opt2._shadow]):
        assert torch.equal(x, y)
    # without EMA: no 'ema_variables'; without an optimizer: the old file
    plain = optimizer_factory['sgd'](learning_rate=1e-3, momentum=0.9)
    plain.init_state(net)
    train.save(net, str(tmp_path / 'p'), 1, plain)
    ck = torch.load(train.latest_checkpoint(str(tmp_path / 'p')),
                    map_location='cpu')
    assert set(ck) == {'variables', 'step', 'optimizer'}
    old = str(tmp_path / 'old')
    train.save(net, old, 7)
    ck = torch.load(train.latest_checkpoint(old), map_location='cpu')
    assert set(ck) == {'variables', 'step'}
    # a checkpoint with neither key still loads; the optimizer starts afresh
    net3 = _net(seed=8)
    opt3 = optimizer_factory['adam'](learning_rate=1e-3, momentum=0.9,
                                     ema_decay=0.75)
    assert train.load(net3, old, opt3) == 7
    assert torch.equal(net3.params, net.params)
    assert opt3._step == 0 and opt3._slots is None and opt3._shadow is None
    assert train.load(_net(), old) == 7


def test_train_flags_default_off_and_bad_values(tmp_path, capsys):
    import train
    a = train.get_arguments([])
    assert a.clip_norm is None and a.ema_decay is None
    a = train.get_arguments(['--clip_norm', '2.5', '--ema_decay', '0.999'])
    assert a.clip_norm == 2.5 and a.ema_decay == 0.999


def test_generate_use_ema_needs_ema_variables(hip_lib, tmp_path, capsys,
                                              monkeypatch):
    import generate
    from wavenet import _lib
    net = _net()
    ck = str(tmp_path / 'model.ckpt-3')
    torch.save({'variables': net.state_dict(), 'step': 3}, ck)
    # refused before any model is built
    monkeypatch.setattr(_lib, 'require_gpu',
                        lambda: pytest.fail('device touched'))
    assert generate.get_arguments([ck]).use_ema is False
    rc = generate.main([ck, '--use_ema', 'true', '--wavenet_params',
                        str(tmp_path / 'missing.json')])
    out = capsys.readouterr().out
    assert rc == 1 and 'ema_variables' in out and '--ema_decay' in out


# ------------------------------------------------- the float64 restatement
@pytest.mark.parametrize('kind', KINDS)
def test_clip_ref_identities(kind):
    rng = np.random.default_rng(0)
    w0 = rng.standard_normal(50)
    g = rng.standard_normal(50)
    norm = math.sqrt(float(np.sum(g * g)))
    assert abs(clip_ref.global_norm(g) - norm) < 1e-12
    assert abs(clip_ref.global_norm(g, 0.5) - 0.5 * norm) < 1e-12
    # below the threshold: factor exactly 1, the step is TFOptimizer's own
    assert clip_ref.clip_factor(norm, 2 * norm) == 1.0
    assert clip_ref.clip_factor(norm, norm) == 1.0
    assert clip_ref.clip_factor(norm, None) == 1.0
    from util import O
    a = clip_ref.ClipEMAOptimizer(kind, 1e-2, 0.9, clip_norm=2 * norm)
    b = O.TFOptimizer(kind, 1e-2, 0.9)
    assert np.array_equal(a.apply(w0, g), b.apply(w0.copy(), g.copy()))
    assert a.last_norm == clip_ref.global_norm(g)
    # above: the scaled gradient's norm is clip_norm
    f = clip_ref.clip_factor(norm, norm / 4)
    assert abs(f - 0.25) < 1e-15
    assert abs(clip_ref.global_norm(g * f) - norm / 4) < 1e-12
    c = clip_ref.ClipEMAOptimizer(kind, 1e-2, 0.9, clip_norm=norm / 4)
    d = O.TFOptimizer(kind, 1e-2, 0.9)
    assert np.allclose(c.apply(w0, g), d.apply(w0.copy(), g * 0.25),
                       rtol=0, atol=1e-15)
    # the 1 / N of the data-parallel average is part of the norm
    e = clip_ref.ClipEMAOptimizer(kind, 1e-2, 0.9, clip_norm=norm / 4)
    same = clip_ref.ClipEMAOptimizer(kind, 1e-2, 0.9, clip_norm=norm / 4)
    assert np.allclose(e.apply(w0, 2 * g, grad_scale=0.5), same.apply(w0, g),
                       rtol=0, atol=1e-15)
    assert abs(e.last_norm - norm) < 1e-12
    # non-finite norm: NaN factor
    assert math.isnan(clip_ref.clip_factor(float('inf'), 1.0))
    assert math.isnan(clip_ref.clip_factor(float('nan'), 1.0))


@pytest.mark.parametrize('kind', KINDS)
def test_clip_ref_shadow_closed_form(kind):
    rng = np.random.default_rng(1)
    w = rng.standard_normal(30)
    decay, k = 0.8, 6
    o = clip_ref.ClipEMAOptimizer(kind, 1e-2, 0.9, clip_norm=1.0,
                                  ema_decay=decay)
    ws = [w.copy()]
    for _ in range(k):
        w = o.apply(w, rng.standard_normal(30))
        ws.append(w.copy())
    closed = decay ** k * ws[0] + (1 - decay) * sum(
        decay ** (k - j) * ws[j] for j in range(1, k + 1))
    assert np.abs(o.shadow - closed).max() < 1e-14
    # decay 0: the shadow is the weights
    z = clip_ref.ClipEMAOptimizer(kind, 1e-2, 0.9, ema_decay=0.0)
    w1 = z.apply(ws[0], rng.standard_normal(30))
    assert np.array_equal(z.shadow, w1)
