"""Training sessions on shared workspaces (wavenet/workspace.py): one model is
called the way train.py calls it -- training steps at changing lengths with
an optimizer step after each, forward-only losses, predict_proba and score in
between, an evaluation under swapped parameters, a longer batch that evicts
the owner, another batch size -- so that most calls run on views carved out of
an owner workspace, with launch plans going from eager to recorded to
replayed while other shapes use the same memory.

The reference of every call is a SEPARATE model for that one shape: launch
plans off, an exactly sized owner workspace, the session model's parameters
copied in before the call.  Every launch decision is a function of
(B, T, variant word), a view starts at offset 0 of its owner's buffers and
every reduction runs in a fixed order, so the contract is BITWISE equality:
the float32 loss, the gradient bucket, and for forward-only calls the logits,
the predict_proba row and the score outputs.  At the stated points the
session model is also held to the float64 oracle with the rule and bounds of
the kind's own tests (test_gpu_model.check_grads and TOL; tests/lc_ctx_ref.py
with test_gpu_lc_context.py's bars for the local-conditioning model;
tests/mol_ref.py with test_gpu_mol_model.py's bars for the models with a
mixture-of-logistics head, whose "predict_proba" is predict_mixture).

Kinds with `draws` also draw per-clip lengths and piece history (train.py's
pieces with their true left context) on every so-manieth call."""
import numpy as np
import pytest
import torch

import lc_ctx_ref
import lc_ref
import mol_ref
from test_gpu_model import (TOL, _ERRLOG, check_grads,  # noqa: F401
                            _dump_errlog)   # (module fixture: grad_errors.json)
from util import (O, TINY, MID, DEFAULT, cfg_with, model_kwargs, build_pair,
                  tree_to_numpy, oracle_grads_at_device_kinks)

pytestmark = pytest.mark.gpu

LC_TOL = 2e-5     # test_gpu_lc_context.py: of each variable's largest entry
LC_DIL = [1, 2, 4, 8, 16, 32, 64, 128, 1, 2]
LC_SCALES, LC_CH, LC_CTX = (4, 5), 12, 2


def _bits(x):
    return x.detach().reshape(1).view(torch.int32)


def _owners(net, training=None):
    return [w for w in net._ws.values() if w.capacity == w.N and
            (training is None or w.training == training)]


def _replayed(ws, tag):
    """a recorded launch plan of pass `tag` exists: the next call replays"""
    return any(k[0] == tag and isinstance(p, list)
               for k, p in ws.plans.items())


class Plain(object):
    """A model the project's float64 oracle restates (oracle/)."""

    def __init__(self, name, cfg, setup=None, draws=(0, 0)):
        self.name, self.cfg, self.B = name, cfg, cfg['batch_size']
        self.gc = cfg.get('global_condition_cardinality')
        self.setup = setup
        # (m, k): the session draws lengths on every m-th training call and
        # history on every k-th (0: never)
        self.draws = draws

    def model(self, first=False, B=None):
        from wavenet import WaveNetModel
        cfg = cfg_with(self.cfg, batch_size=B or self.B)
        if first:       # non-zero biases, the oracle's own initialisation
            net = build_pair(cfg)[0]
        else:
            net = WaveNetModel(**model_kwargs(cfg))
        if self.setup:
            self.setup(net)
        return net

    def inputs(self, rng, B, T):
        inp = dict(audio=rng.uniform(-1, 1, (B, T)).astype(np.float32))
        if self.gc:
            inp['ids'] = rng.integers(0, self.gc, B).astype(np.int32)
        return inp

    def kwargs(self, net, inp, host):
        """(positional, keyword) arguments of loss / score for `inp`; host:
        the GC ids as a fresh host array instead of a device tensor"""
        ids = inp.get('ids')
        if ids is not None:
            ids = ids.copy() if host else torch.as_tensor(ids).cuda()
        return (torch.from_numpy(inp['audio']).cuda(), ids), {}

    def proba_args(self, net, inp):
        codes = O.mu_law_encode(inp['audio'], self.cfg['quantization_channels'])
        return (codes, inp.get('ids')), {}

    def anchor(self, net, inp, loss, tag):
        cfg = cfg_with(self.cfg, batch_size=inp['audio'].shape[0])
        var = tree_to_numpy(net.variables)
        ref_loss, ref_g, _, _ = oracle_grads_at_device_kinks(
            net, cfg, var, inp['audio'], inp.get('ids'))
        assert abs(float(loss) - ref_loss) < TOL, (tag, float(loss), ref_loss)
        check_grads(net, ref_g, tag='workspace_sequence/' + tag)
        print('%s: loss %.7f, float64 %.7f; worst gradient error %.3g of the '
              'variable\'s largest entry'
              % (tag, float(loss), ref_loss,
                 max(e / s for e, s in
                     _ERRLOG['workspace_sequence/' + tag].values() if s > 0)))


class LcUpCtx(object):
    """Local conditioning from frames: context 2, learned upsampler, GC."""
    name, B, gc, Q = 'lc_up_ctx_gc', 2, 3, 64
    draws = (2, 0)

    def model(self, first=False, B=None):
        from wavenet import WaveNetModel
        net = WaveNetModel(B or self.B, LC_DIL, 2, 32, 32, 64,
                           quantization_channels=self.Q, use_biases=True,
                           seed=3, global_condition_channels=self.gc,
                           global_condition_cardinality=self.gc,
                           local_condition_channels=LC_CH,
                           local_condition_upsample_scales=LC_SCALES,
                           local_condition_context=LC_CTX)
        if first:
            # non-zero biases, LC weights large enough that the rows matter,
            # a context filter away from its identity initialisation
            g = torch.Generator().manual_seed(11)
            with torch.no_grad():
                for n, v in net.named_variables():
                    last = n.split('/')[-1]
                    r = torch.randn(v.shape, generator=g, dtype=torch.float64)
                    if '/lc_context/' in n:
                        v.copy_((r / np.sqrt(v.shape[0] * v.shape[1])).float())
                    elif '/lc_upsample/' in n:
                        v.copy_((0.6 * r).float())
                    elif 'bias' in last:
                        v.copy_((0.1 * r).float())
                    elif last.startswith('lc_'):
                        v.copy_((0.3 * r).float())
        return net

    def inputs(self, rng, B, T):
        hop = int(np.prod(LC_SCALES))
        offs = rng.integers(0, 3 * hop, B)
        F = int((offs.max() + T - 1) // hop + 1)
        return dict(audio=rng.uniform(-1, 1, (B, T)).astype(np.float32),
                    ids=rng.integers(0, self.gc, B).astype(np.int32),
                    frames=rng.standard_normal((B, F, LC_CH)).astype(np.float32),
                    offs=[int(o) for o in offs])

    def kwargs(self, net, inp, host):
        ids = inp['ids'].copy() if host else torch.as_tensor(inp['ids']).cuda()
        return (torch.from_numpy(inp['audio']).cuda(), ids), dict(
            local_condition_batch=inp['frames'],
            local_condition_offset=inp['offs'])

    def proba_args(self, net, inp):
        T = inp['audio'].shape[1]
        rows = net.upsample_local_condition(inp['frames'], T, inp['offs'])
        return (O.mu_law_encode(inp['audio'], self.Q), inp['ids']), \
            dict(local_condition=rows)

    def anchor(self, net, inp, loss, tag):
        B, T = inp['audio'].shape
        ref_loss, ref_g = lc_ctx_ref.loss_and_grads(
            lc_ref.model_tree(net), LC_DIL, O.mu_law_encode(inp['audio'], self.Q),
            inp['frames'], inp['offs'], LC_SCALES, gc_ids=inp['ids'],
            use_biases=True, quantization_channels=self.Q,
            relu_masks=lc_ref.device_relu_masks(net, B, T))
        assert abs(float(loss) - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
        got = dict(lc_ref.flatten(lc_ref.model_tree(net, grads=True)))
        ref = dict(lc_ref.flatten(ref_g))
        assert sorted(got) == sorted(ref)
        assert np.abs(ref['/lc_context/filter']).max() > 0
        bad = []
        for k in sorted(ref):
            # (test_gpu_lc_context._bad_grads: an upsampler layer's one-float
            # bias gradient is held to its layer's largest entry)
            scale = np.abs(ref[k]).max()
            if k.startswith('/lc_upsample/') and k.endswith('/bias'):
                scale = max(scale,
                            np.abs(ref[k[:-len('bias')] + 'filter']).max())
            err = np.abs(got[k] - ref[k]).max()
            _ERRLOG.setdefault('workspace_sequence/' + tag, {})[k] = \
                (float(err), float(scale))
            if not err <= LC_TOL * max(scale, 1e-30):
                bad.append((k, float(err), float(scale)))
        assert not bad, (tag, bad[:6])


MOL_TOL = 2e-5    # test_gpu_mol_model.py: of each variable's largest entry
MOL_DIL = MID['dilations']
MOL_SCALES, MOL_LC = (2, 4), 5


class Mixture(object):
    """A scalar-input model with a mixture-of-logistics head (wavenet/mol.py):
    K components, Q = 3 Kp logit columns; GC, or frames through the learned
    upsampler (context 1) at drawn offsets."""
    B = 2

    def __init__(self, name, K, ifw, gc=None, lc_up=False, draws=(2, 3),
                 lc_gain=(0.5, 0.3)):
        self.name, self.K, self.ifw, self.gc = name, K, ifw, gc
        self.lc_up, self.draws = lc_up, draws
        # standard deviation of the first model's upsampler and LC weights
        self.LC_GAIN = lc_gain

    def model(self, first=False, B=None):
        from wavenet import WaveNetModel
        kw = {}
        if self.gc:
            kw.update(global_condition_channels=self.gc,
                      global_condition_cardinality=self.gc)
        if self.lc_up:
            kw.update(local_condition_channels=MOL_LC,
                      local_condition_upsample_scales=MOL_SCALES,
                      local_condition_context=1)
        net = WaveNetModel(B or self.B, MOL_DIL, 2, 32, 32, 64,
                           quantization_channels=64, use_biases=True,
                           scalar_input=True, initial_filter_width=self.ifw,
                           seed=3, output_mixture=self.K, **kw)
        assert net.Q == 3 * net.mol_Kp == 3 * ((self.K + 3) // 4 * 4)
        if first:
            # test_gpu_mol_model._model: non-zero biases, LC weights large
            # enough that the rows matter, scales round e^-2 of full scale
            g = torch.Generator().manual_seed(14)
            with torch.no_grad():
                for n, v in net.named_variables():
                    last = n.split('/')[-1]
                    r = torch.randn(v.shape, generator=g, dtype=torch.float64)
                    if '/lc_upsample/' in n or '/lc_context/' in n:
                        v.copy_((self.LC_GAIN[0] * r).float())
                    elif 'bias' in last:
                        v.copy_((0.1 * r).float())
                    elif last.startswith('lc_'):
                        v.copy_((self.LC_GAIN[1] * r).float())
                Kp = net.mol_Kp
                net.variables['postprocessing']['postprocess2_bias'][
                    2 * Kp:2 * Kp + self.K] -= 2.0
        return net

    def inputs(self, rng, B, T):
        # sine + noise (util.synth_audio's clips, drawn from the session's rng)
        t = np.arange(T)[None, :]
        f = rng.uniform(80.0, 400.0, (B, 1))
        x = 0.5 * np.sin(2 * np.pi * f * t / 16000.0 +
                         rng.uniform(0, 2 * np.pi, (B, 1))) + \
            0.05 * rng.standard_normal((B, T))
        inp = dict(audio=np.clip(x, -1, 1).astype(np.float32))
        if self.gc:
            inp['ids'] = rng.integers(0, self.gc, B).astype(np.int32)
        if self.lc_up:
            hop = int(np.prod(MOL_SCALES))
            offs = rng.integers(0, 3 * hop, B)
            F = int((offs.max() + T - 1) // hop + 1)
            inp['frames'] = rng.standard_normal((B, F, MOL_LC)).astype(
                np.float32)
            inp['offs'] = [int(o) for o in offs]
        return inp

    def kwargs(self, net, inp, host):
        ids = inp.get('ids')
        if ids is not None:
            ids = ids.copy() if host else torch.as_tensor(ids).cuda()
        kw = {}
        if self.lc_up:
            kw = dict(local_condition_batch=inp['frames'],
                      local_condition_offset=inp['offs'])
        return (torch.from_numpy(inp['audio']).cuda(), ids), kw

    def proba_args(self, net, inp):
        """predict_mixture's: the float audio, the ids, the LC rows"""
        kw = {}
        if self.lc_up:
            kw['local_condition'] = net.upsample_local_condition(
                inp['frames'], inp['audio'].shape[1], inp['offs'])
        return (inp['audio'], inp.get('ids')), kw

    def anchor(self, net, inp, loss, tag):
        from wavenet import mol
        B, T = inp['audio'].shape
        lv, x = mol.levels_reference(inp['audio'])
        ref_loss, ref_g, _, _ = mol_ref.network(
            lc_ref.model_tree(net), MOL_DIL, x, mol_ref.targets(lv),
            float(B * T), (self.K, net.mol_log_scale_min),
            lc=inp.get('frames'), scales=MOL_SCALES if self.lc_up else None,
            gc_ids=inp.get('ids'), use_biases=True,
            relu_masks=lc_ref.device_relu_masks(net, B, T),
            offsets=inp.get('offs', 0))
        assert abs(float(loss) - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), \
            (tag, float(loss), ref_loss)
        got = dict(lc_ref.flatten(lc_ref.model_tree(net, grads=True)))
        ref = dict(lc_ref.flatten(ref_g))
        assert sorted(got) == sorted(ref)
        bad, worst = [], 0.0
        for k in sorted(ref):
            scale = np.abs(ref[k]).max()
            err = np.abs(got[k] - ref[k]).max()
            _ERRLOG.setdefault('workspace_sequence/' + tag, {})[k] = \
                (float(err), float(scale))
            worst = max(worst, err / max(scale, 1e-30))
            if not err <= MOL_TOL * max(scale, 1e-30):
                bad.append((k, float(err), float(scale)))
        print('%s: loss %.7f, float64 %.7f; worst gradient error %.3g of the '
              'variable\'s largest entry' % (tag, float(loss), ref_loss, worst))
        assert not bad, (tag, bad[:6])


class Session(object):
    """The session model, its optimizer, and one reference model per shape."""

    def __init__(self, kind, opt='adam', seed=0):
        from wavenet import optimizer_factory
        self.kind, self.B = kind, kind.B
        self.net = kind.model(first=True)
        assert self.net.use_launch_plans
        if opt == 'adam':
            self.opt = optimizer_factory['adam'](
                learning_rate=1e-3, momentum=0.9, ema_decay=0.9)
        else:
            self.opt = optimizer_factory['sgd'](learning_rate=0.01,
                                                momentum=0.9)
        self.refs = {}
        self.rng = np.random.default_rng(seed)
        self.ncalls = self.ntrain = 0

    def set_batch(self, B):
        self.B = self.net.batch_size = B

    def ref(self, T, training, params=None):
        key = (self.B, T, training)
        if key not in self.refs:
            r = self.kind.model(B=self.B)
            r.use_launch_plans = False
            self.refs[key] = r
        r = self.refs[key]
        with torch.no_grad():
            r.params.copy_(self.net.params if params is None else params)
        return r

    def _exact(self, r, T, training):
        ws = r._ws[(self.B, T, training)]
        assert ws.capacity == ws.N == self.B * T and not ws.plans
        return ws

    def _history(self, n, T, host):
        """h[b] drawn from [0, n[b]] (n: the lengths, T without them), 0 for
        at least one clip: dict(history=h), or {} without `history`"""
        n = np.full(self.B, T) if n is None else np.asarray(n)
        h = self.rng.integers(0, n + 1).astype(np.int64)
        h[self.rng.integers(0, self.B)] = 0
        return dict(history=h.copy() if host else torch.as_tensor(h))

    def train(self, T, lengths=None, host=False, anchor=None, replays=None,
              step=True, history=None):
        """One training call at length T against its reference, then (step)
        an optimizer step.  lengths: True draws them; history: True draws it
        (after the lengths); host: GC ids, lengths and history from fresh
        host arrays; anchor: also against float64, under that tag; replays:
        assert that the call does (not) replay a plan."""
        net, kind, B = self.net, self.kind, self.B
        inp = kind.inputs(self.rng, B, T)
        n = None
        if lengths:
            n = np.append(self.rng.integers(1, T + 1, B - 1), T).astype(np.int64)
            n = n.copy() if host else torch.as_tensor(n)
        hkw = self._history(n, T, host) if history else {}
        if replays is not None:
            ws = net._ws.get((B, T, True))
            assert ws is not None and _replayed(ws, 'fwd') == replays
        r = self.ref(T, True)
        out = []
        for m in (net, r):
            a, kw = kind.kwargs(m, inp, host)
            out.append(m.loss(*a, lengths=n, **dict(kw, **hkw)))
        torch.cuda.synchronize()
        what = (kind.name, 'train', B, T, self.ncalls,
                None if n is None else np.asarray(n).tolist(),
                [np.asarray(h).tolist() for h in hkw.values()])
        assert torch.equal(_bits(out[0]), _bits(out[1])), \
            what + (float(out[0]), float(out[1]))
        assert bool(torch.isfinite(out[0]))
        assert torch.equal(net.grads, r.grads), what
        self._exact(r, T, True)
        if anchor:
            assert n is None and not hkw
            kind.anchor(net, inp, out[0], '%s/%s' % (kind.name, anchor))
        if step:
            self.opt.minimize(out[0])
        self.ncalls += 1
        self.ntrain += 1
        return net._ws[(B, T, True)]

    def forward_loss(self, T, history=None):
        """loss(backward=False): the loss and the logits, bitwise."""
        net, kind, B = self.net, self.kind, self.B
        inp = kind.inputs(self.rng, B, T)
        hkw = self._history(None, T, False) if history else {}
        r = self.ref(T, False)
        out = []
        for m in (net, r):
            a, kw = kind.kwargs(m, inp, False)
            out.append(m.loss(*a, backward=False, **dict(kw, **hkw)))
        torch.cuda.synchronize()
        what = (kind.name, 'forward', B, T, self.ncalls)
        assert torch.equal(_bits(out[0]), _bits(out[1])), what
        ws = net._ws[(B, T, False)]
        assert torch.equal(ws.logits, self._exact(r, T, False).logits), what
        self.ncalls += 1
        return ws

    def _proba(self, m, inp):
        """predict_proba, or a mixture model's predict_mixture, and the
        probability mass it states"""
        pa, pkw = self.kind.proba_args(m, inp)
        if m.mol_K:
            p = m.predict_mixture(*pa, **pkw)
            assert p.shape == (3, m.mol_K) and bool(torch.isfinite(p).all())
            return p, p[0].double().exp().sum()
        p = m.predict_proba(*pa, **pkw)
        return p, p.sum()

    def proba_and_score(self, T, shadow=None, lengths=False, history=None):
        """predict_proba (predict_mixture) and score at length T, bitwise;
        shadow: with the session model's parameters swapped for it (the
        reference holds it)."""
        import contextlib
        from wavenet import evaluate
        net, kind, B = self.net, self.kind, self.B
        inp = kind.inputs(self.rng, B, T)
        n = None
        if lengths:
            n = np.append(self.rng.integers(1, T + 1, B - 1), T)
        hkw = self._history(n, T, True) if history else {}
        r = self.ref(T, False, params=shadow)
        swap = evaluate.parameters_swapped(net, shadow) \
            if shadow is not None else contextlib.nullcontext()
        before = net.params.clone()
        with swap:
            p, mass = self._proba(net, inp)
            a, kw = kind.kwargs(net, inp, False)
            s = net.score(*a, lengths=n, per_sample=True, **dict(kw, **hkw))
        assert torch.equal(net.params, before)
        p_ref, _ = self._proba(r, inp)
        a, kw = kind.kwargs(r, inp, False)
        s_ref = r.score(*a, lengths=n, per_sample=True, **dict(kw, **hkw))
        torch.cuda.synchronize()
        what = (kind.name, 'proba/score', B, T, self.ncalls)
        assert torch.equal(p, p_ref) and abs(float(mass) - 1) < 1e-5, what
        for name, x, y in zip(s._fields, s, s_ref):
            if name == 'correct' and net.mol_K:
                # (an arg-max is not defined for a mixture head)
                assert x is None and y is None, what
                continue
            assert torch.equal(x, y), what + (name,)
        assert bool(torch.isfinite(s.nll).all()) and int(s.count.sum()) > 0
        ws = net._ws[(B, T, False)]
        assert torch.equal(ws.logits, self._exact(r, T, False).logits), what
        self.ncalls += 2
        return ws


def _default_checks(net, ws):
    path = net._step_path(ws, True)
    assert path.fwd == 'stack_skip' and path.bwd == 'stack', path
    assert path.overlap_tn and ws.stack_rows == 16


def _blocked_checks(net, ws):
    assert net.blocked and net._step_path(ws, True).bwd == 'blocked'


def _k3_checks(net, ws):
    path = net._step_path(ws, True)
    assert path.fwd == path.bwd == 'layer_k', path
    assert ws.legacy and ws.TH is not None and ws.da is not None


def _stack_checks(net, ws):
    path = net._step_path(ws, True)
    assert path.fwd.startswith('stack') and path.bwd.startswith('stack'), path


def _scalar_stack_checks(net, ws):
    path = net._step_path(ws, True)
    assert path.fwd in ('stack', 'stack_skip') and path.bwd == 'stack', path
    assert net.scalar_input and ws.audio is not None
    assert path.causal_wgrad == 'scalar', path


def _scalar_lc_checks(net, ws):
    path = net._step_path(ws, True)
    assert path.fwd == path.bwd == 'stack_lc', path
    assert net.scalar_input and ws.audio is not None
    assert path.causal_wgrad == 'scalar', path


# (kind, (T_A, T_b, T_c, T_D), forward-only lengths, proba / score length,
#  the launches the kind is here for, asserted on every training workspace)
SESSIONS = [
    (Plain('mid_gc', cfg_with(MID, batch_size=2, global_condition_channels=4,
                              global_condition_cardinality=5)),
     (608, 333, 21, 1100), (450, 77), 211, _stack_checks),
    (Plain('default', cfg_with(DEFAULT, batch_size=1)),
     (800, 417, 23, 1300), (512, 90), 300, _default_checks),
    (Plain('mid_r64', cfg_with(MID, batch_size=2, residual_channels=64,
                               dilation_channels=64)),
     (416, 250, 19, 650), (320, 45), 130, _blocked_checks),
    (Plain('tiny_k3', cfg_with(TINY, batch_size=2, filter_width=3)),
     (512, 290, 30, 900), (401, 64), 150, _k3_checks),
    (LcUpCtx(), (640, 350, 27, 1000), (480, 100), 222, _stack_checks),
    # scalar input: a 32-tap causal layer, longer than the clip at T_c; with
    # a mixture head 36 and 96 logit columns (K = 10: Kp = 12; K = 32: eight
    # components per lane), the second behind the learned LC upsampler
    (Plain('scalar_softmax_gc',
           cfg_with(MID, batch_size=2, scalar_input=True,
                    initial_filter_width=32, global_condition_channels=4,
                    global_condition_cardinality=5), draws=(2, 3)),
     (576, 301, 25, 1050), (430, 70), 190, _scalar_stack_checks),
    (Mixture('mol_k10_gc', 10, 32, gc=3),
     (640, 345, 29, 1200), (470, 85), 205, _scalar_stack_checks),
    # (LC gains: with test_gpu_mol_model._model's 0.5 / 0.3, made for five
    # layers, these 14 layers behind a two-tap causal layer are conditioned
    # so badly that the float64 network restated in float32 -- torch on the
    # CPU, nothing of the device -- is itself 4.3e-6 of a variable's largest
    # entry off at T_A, a fifth of the bar; at a quarter of them it is
    # 1.5e-6 at the most, as for the models without LC)
    (Mixture('mol_k32_lc_up', 32, 2, lc_up=True, lc_gain=(0.125, 0.075)),
     (544, 275, 22, 980), (410, 60), 170, _scalar_lc_checks),
]


@pytest.mark.parametrize('kind,train_T,fwd_T,T_p,checks', SESSIONS,
                         ids=[s[0].name for s in SESSIONS])
def test_training_session_on_shared_workspaces(hip_lib, kind, train_T, fwd_T,
                                               T_p, checks):
    T_A, T_b, T_c, T_D = train_T
    assert T_c < 32 <= T_b < T_A < T_D and T_b % 32 and T_A % 32 == 0
    every_n, every_h = kind.draws
    s = Session(kind)
    net, B = s.net, s.B
    # forward-only lengths, never the owner's own (phase 2: new ones, so that
    # they are carved out of the new owner; T_A itself among them)
    fwd_cycle = [T_b, fwd_T[0], T_c, fwd_T[1]]

    def train(T, **kw):
        # (kind.draws: lengths on every second call of the LC and the
        # scalar-input models, history on every third, except at an anchor)
        if every_n and s.ntrain % every_n == 1 and not kw.get('anchor'):
            kw.setdefault('lengths', True)
        if every_h and s.ntrain % every_h == 2 and not kw.get('anchor'):
            kw.setdefault('history', True)
        ws = s.train(T, **kw)
        if s.ntrain % 2 == 0:
            # a forward-only view of the training owner, at another length
            Tf = [t for t in fwd_cycle if t != T][(s.ntrain // 2) % 3]
            fw = s.forward_loss(Tf, history=every_h and s.ntrain % 4 == 0)
            own, = _owners(net, True)
            assert fw.capacity == own.N != fw.N
            assert fw.X.data_ptr() == own.X.data_ptr()
        return ws

    # ---- phase 1: owner T_A, views T_b and T_c
    owner = train(T_A, anchor='first', replays=None)
    assert owner.capacity == owner.N and _owners(net) == [owner]
    checks(net, owner)
    for rnd in range(3):
        for T in (T_b, T_A, T_c):
            if rnd == 1 and T == T_b:
                # GC ids and lengths staged from fresh host arrays; then the
                # same shape without lengths
                train(T, lengths=True, host=True)
                ws = train(T, lengths=False, host=True, replays=True)
            elif rnd == 2 and T == T_b:
                ws = train(T, anchor='phase1_replayed_view', replays=True)
            else:
                ws = train(T)
            assert (ws.capacity == ws.N) == (T == T_A)
            assert ws.X.data_ptr() == owner.X.data_ptr()
            checks(net, ws)
        s.proba_and_score(T_p, lengths=rnd == 1, history=every_h and rnd > 0)
    assert _owners(net) == [owner]
    # ---- phase 2: T_D outgrows the owner; T_A comes back as a view
    fwd_cycle = [T_A, fwd_T[0] + 5, T_c + 5, fwd_T[1] + 5]
    big = train(T_D)
    assert big.capacity == big.N == B * T_D and _owners(net, True) == [big]
    assert [w for w in net._ws.values() if w.training] == [big]
    assert big is not owner
    for rnd in range(3):
        for T in (T_b, T_D, T_A, T_c):
            if rnd == 2 and T == T_A:
                ws = train(T, anchor='phase2_replayed_view', replays=True)
            else:
                ws = train(T)
            assert (ws.capacity == ws.N) == (T == T_D)
            assert ws.capacity == big.N
            assert ws.X.data_ptr() == big.X.data_ptr()
            checks(net, ws)
        if rnd == 1:
            # as training.validate with --validate_ema: score with the EMA
            # shadow swapped in; the next training call is bitwise again
            s.proba_and_score(T_p, shadow=s.opt.ema_flat(net).clone(),
                              history=every_h)
        else:
            s.proba_and_score(T_p, history=every_h and rnd == 2)
    # ---- the end state
    net.check_device_errors()
    for T in train_T:
        ws = net._ws[(B, T, True)]
        assert _replayed(ws, 'fwd'), T
        assert _replayed(ws, 'bwd') == (not net.blocked), T
    assert [w for w in net._ws.values() if w.capacity == w.N] == [big]
    assert any(_replayed(w, 'fwd') for w in net._ws.values()
               if not w.training)
    print('%s: %d calls compared bitwise (%d training)'
          % (kind.name, s.ncalls, s.ntrain))


@pytest.mark.parametrize('waves,gc', [(0, False), (4, False), (0, True)],
                         ids=['default', 'waves4', 'default_gc'])
def test_views_across_the_tile_row_boundary(hip_lib, waves, gc):
    """An owner on 32-row tiles, views on 16-row tiles inside its memory
    (with GC the per-tile column sums too: two tile heights, one buffer)."""
    from wavenet._lib import stack_variant
    B, T_s = 4, 1000
    T_hi = 32
    while hip_lib.wn_stack_tile_rows(B, T_hi, 0) != 32:
        T_hi += 32
    T_lo = T_hi - 32
    assert hip_lib.wn_stack_tile_rows(B, T_lo, 0) == 16 and T_s < T_lo
    variant = stack_variant(waves=waves)

    def setup(net):
        net.stack_variant = variant
    extra = dict(global_condition_channels=4,
                 global_condition_cardinality=5) if gc else {}
    kind = Plain('mid_B4_tile_boundary_' + ('waves4' if waves else 'default')
                 + ('_gc' if gc else ''),
                 cfg_with(MID, batch_size=B, **extra), setup)
    s = Session(kind, opt='sgd')
    net = s.net
    owner = s.train(T_hi)
    rows = {T_hi: 32, T_lo: 16, T_s: 16}
    seen = {}
    for rnd in range(3):
        for T in (T_lo, T_hi, T_s):
            last = rnd == 2 and T == T_lo
            ws = s.train(T, anchor='last_T_lo' if last else None,
                         replays=True if last else None)
            assert ws.stack_variant == variant and ws.stack_rows == rows[T]
            assert ws.X.data_ptr() == owner.X.data_ptr()
            path = net._step_path(ws, True)
            assert path.fwd == path.bwd == 'stack', path
            seen[T] = (ws, path)
    assert _owners(net) == [owner] and owner is seen[T_hi][0]
    # the 16-row view's TN GEMMs run on the side stream, on the owner's
    # slabs_tn; the owner's own run on the main stream
    assert seen[T_lo][1].overlap_tn and not seen[T_hi][1].overlap_tn
    v = seen[T_lo][0]
    assert v.slabs_tn.data_ptr() == owner.slabs_tn.data_ptr()
    assert v.region['layers_stack'].count <= owner.lslabs.shape[1]
    if waves == 4:
        # (the view's launch writes more slabs per layer than the owner's)
        assert v.region['layers_stack'].count > \
            owner.region['layers_stack'].count
    for T in rows:
        assert _replayed(seen[T][0], 'fwd') and _replayed(seen[T][0], 'bwd')
    net.check_device_errors()
    print('%s: %d calls compared bitwise' % (kind.name, s.ncalls))


def test_batch_size_alternation_evicts_and_recovers(hip_lib):
    kind = Plain('mid_gc_batch_alternation',
                 cfg_with(MID, batch_size=2, global_condition_channels=4,
                          global_condition_cardinality=5))
    s = Session(kind, opt='sgd')
    net = s.net
    for B, lengths in ((2, (600, 300)), (3, (250, 420)), (2, (600, 300))):
        s.set_batch(B)
        for T in lengths:
            ws = s.train(T)
            assert ws.B == B
            own = _owners(net, True)
            assert len(own) == 1 and own[0].B == B
            assert all(w.B == B for w in net._ws.values() if w.training)
        # (the second length: a view at B = 2, a new owner at B = 3)
        assert (ws.capacity == ws.N) == (B == 3)
    net.check_device_errors()
    print('%s: %d calls compared bitwise' % (kind.name, s.ncalls))
