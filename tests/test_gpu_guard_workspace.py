"""The whole training pass on a view carved out of a larger owner workspace,
with the owner's memory behind every buffer of the view used as a guard band.

workspace.get carves a shorter call out of a resident owner as the flat prefix
of each named buffer (getattr(parent, name).reshape(-1)[:n]), so what the
owner holds beyond n is memory no launch of the view may touch.  Per (kind, B,
T_view): the owner is built by one call at T_owner = 2 T_view + 37; the tail
of every tensor of the owner beyond what the (B, T_view) views take is filled
-- floats with the NaN 0x7FC0A5A5, code buffers with Q - 1, flag / control /
mask buffers with a word no epoch or length takes; then the session of
tests/test_gpu_workspace_sequence.py runs in miniature at T_view: three
training calls (launch plans eager, recorded, replayed), a forward-only loss,
score(per_sample=True) and predict_proba.

  * WRITES: after every call every tail is bit-identical to what was written.
  * READS: the view calls are repeated with the float tails at 0.0 and the
    code tails at 0; the loss bits, the gradient bucket, the logits and the
    score / predict_proba outputs equal the first run's bit for bit.  (A read
    that changes no result is invisible: tests/guard.py.)

A bounded wait of a stack launch that expires turns the loss NaN: the test
asserts finite losses and is never to be retried for that.

Known limit: the planes of one buffer are contiguous in a view, so a spill
from plane l into plane l + 1 is caught for the last plane only
(tests/test_gpu_guard_entries.py gives every plane its own bands).  Buffers
whose size does not depend on T have no tail; they are printed once per
kind."""
import numpy as np
import pytest
import torch

import guard
from test_gpu_workspace_sequence import Plain, LcUpCtx
from util import TINY, cfg_with

pytestmark = pytest.mark.gpu

CODES = ('q', 'q_tgt')                   # values that become addresses
# checked for writes only; the fill is a word no live epoch or length takes
WRITE_ONLY = ('stack_flags', 'stack_flags_b', 'stack_ctl', 'stack_ctl_b',
              'xent_mask', 'xent_hist', 'gc_ids', 'lc_off')
INT_SENTINEL = 0x5A5A5A5A

# remainder 1 and tile - 1 of T and of B * T for the 16-, 32- and 128-row
# tiles, B in {1, 3}:  17 = 16 + 1 (3 * 17 = 51 = 32 + 19), 33 = 32 + 1
# (3 * 33 = 99 = 128 - 29), 129 = 128 + 1 (387 = 3 * 128 + 3), 159 = 160 - 1 =
# 128 + 31 (477 = 480 - 3: 16 - 3, 32 - 3); 2: below every shift of a
# three-tap filter and below the shift of every dilation but 1
T_VIEWS = (2, 17, 33, 129, 159)


def _rows(rows):
    def setup(net):
        from wavenet._lib import stack_variant
        net.stack_variant = stack_variant(rows=rows)

    def check(net, ws, path):
        assert ws.stack_rows == rows and ws.stack_bwd and net._stack_bwd_ok()
        assert path.fwd.startswith('stack') and path.bwd == 'stack', path
    return setup, check


def _perlayer_setup(net):
    net.stack_fwd = net.stack_bwd = False


def _perlayer_check(net, ws, path):
    assert not net.stack_fwd and not net._stack_bwd_ok() and not ws.stack_bwd
    assert path.fwd == 'layer' and path.bwd == 'layer2', path   # wn_layer_fwd / _bwd2


def _k3_check(net, ws, path):
    assert path.fwd == path.bwd == 'layer_k', path
    assert ws.legacy and ws.TH is not None and ws.da is not None


def _scalar_check(net, ws, path):
    assert net.scalar_input and ws.audio is not None
    assert path.causal_wgrad == 'scalar', path


class TinyMixture(Plain):
    """TINY with scalar input and a mixture-of-logistics head (K = 4: 12
    logit columns), every call with drawn lengths and history: the masked and
    windowed branches of wn_mol_quantize / wn_mol_loss / wn_mol_score."""

    def model(self, first=False, B=None):
        from wavenet import WaveNetModel
        from util import model_kwargs
        net = WaveNetModel(**model_kwargs(cfg_with(self.cfg,
                                                   batch_size=B or self.B)))
        if first:       # (test_gpu_mol_model._model)
            g = torch.Generator().manual_seed(5)
            with torch.no_grad():
                for n, v in net.named_variables():
                    if 'bias' in n.split('/')[-1]:
                        v.copy_(0.1 * torch.randn(v.shape, generator=g))
                Kp, K = net.mol_Kp, net.mol_K
                net.variables['postprocessing']['postprocess2_bias'][
                    2 * Kp:2 * Kp + K] -= 2.0
        return net

    def inputs(self, rng, B, T):
        inp = Plain.inputs(self, rng, B, T)
        n = rng.integers(1, T + 1, B)
        if B > 1:
            n[-1] = T
        h = rng.integers(0, n + 1)
        if (n - h).sum() == 0:
            h[-1] = 0
        inp.update(lengths=n.astype(np.int64), history=h.astype(np.int64))
        return inp

    def kwargs(self, net, inp, host):
        a, _ = Plain.kwargs(self, net, inp, host)
        return a, dict(lengths=inp['lengths'], history=inp['history'])

    def proba_args(self, net, inp):
        """predict_mixture's"""
        return (inp['audio'], inp.get('ids')), {}


def _mixture_check(net, ws, path):
    _scalar_check(net, ws, path)
    assert net.mol_K == 4 and net.Q == 12 and ws.logits.shape[1] == 12


def _gc_check(net, ws, path):
    assert path.bwd == 'stack', path
    for name in ('tilesum_buf', 'dsum_part', 'gc_part'):
        assert getattr(ws, name) is not None, name


def _blocked_check(net, ws, path):
    assert net.blocked and path.fwd == path.bwd == 'blocked', path
    for name in ('pslabs', 'dzb', 'pre'):
        assert getattr(ws, name) is not None, name


def _rp_check(net, ws, path):
    assert net.residual_postproc and ws.total is not None and \
        ws.c1 is not None and ws.dh2 is not None


def _lc_check(net, ws, path):
    assert path.fwd == 'stack_lc' and path.bwd == 'stack_lc', path
    assert ws.stack_rows == 32


_R16, _R32 = _rows(16), _rows(32)
GC = dict(global_condition_channels=4, global_condition_cardinality=5)
# (name, kind, setup(net) or None, check(net, training view, its StepPath))
KINDS = [
    ('tiny_rows16', Plain('tiny_rows16', cfg_with(TINY, batch_size=1)),
     _R16[0], _R16[1]),
    ('tiny_rows32', Plain('tiny_rows32', cfg_with(TINY, batch_size=1)),
     _R32[0], _R32[1]),
    ('tiny_perlayer', Plain('tiny_perlayer', cfg_with(TINY, batch_size=1)),
     _perlayer_setup, _perlayer_check),
    ('tiny_k3', Plain('tiny_k3', cfg_with(TINY, batch_size=1, filter_width=3)),
     None, _k3_check),
    ('tiny_scalar', Plain('tiny_scalar', cfg_with(
        TINY, batch_size=1, scalar_input=True, initial_filter_width=4)),
     None, _scalar_check),
    ('tiny_mixture', TinyMixture('tiny_mixture', cfg_with(
        TINY, batch_size=1, scalar_input=True, initial_filter_width=4,
        output_mixture=4)),
     None, _mixture_check),
    ('tiny_gc', Plain('tiny_gc', cfg_with(TINY, batch_size=1, **GC)),
     None, _gc_check),
    ('tiny_r64', Plain('tiny_r64', cfg_with(
        TINY, batch_size=1, residual_channels=64, dilation_channels=64)),
     None, _blocked_check),
    ('tiny_rp', Plain('tiny_rp', cfg_with(TINY, batch_size=1,
                                          residual_postproc=True)),
     None, _rp_check),
    ('lc_up_ctx_gc', LcUpCtx(), None, _lc_check),
]

_printed = set()


def _tensors(ws):
    return {k: v for k, v in vars(ws).items() if isinstance(v, torch.Tensor)}


def _tails(owner, views):
    """[(names, flat int view of the owner's memory beyond the views' use,
    kind of fill)] and the names without a tail.  Attributes that alias one
    allocation (tilesum, tilesum16, tilesum_buf) form one entry: the largest
    alias of the owner beyond the largest of the views."""
    groups = {}
    for name, t in _tensors(owner).items():
        groups.setdefault(t.data_ptr(), []).append(name)
    tails, none = [], []
    for ptr, names in groups.items():
        big = max((getattr(owner, n) for n in names), key=lambda t: t.numel())
        assert big.is_contiguous() and big.element_size() == 4, names
        used = 0
        for v in views:
            for n, t in _tensors(v).items():
                if t.data_ptr() == ptr:
                    assert t.dtype == big.dtype, (n, names)
                    used = max(used, t.numel())
        names = tuple(sorted(names))
        if used >= big.numel():
            none.append('|'.join(names))
            continue
        assert used > 0 or not any(hasattr(v, n) for v in views
                                   for n in names), names
        flat = big.reshape(-1)[used:]
        if big.dtype == torch.float32:
            fill = 'float'
        elif any(n in CODES for n in names):
            fill = 'code'
        else:
            assert all(n in WRITE_ONLY for n in names), \
                'an integer buffer the test does not know: %s' % (names,)
            fill = 'write_only'
        tails.append((names, flat.view(torch.int32), fill))
    return tails, sorted(none)


def _fill(tails, variant, Q):
    for names, words, fill in tails:
        if fill == 'float':
            words.fill_(guard.NAN32 if variant == 'A' else 0)
        elif fill == 'code':
            words.fill_(Q - 1 if variant == 'A' else 0)
        else:
            words.fill_(INT_SENTINEL)


def _check(tails, variant, Q, what):
    for names, words, fill in tails:
        want = {'float': guard.NAN32 if variant == 'A' else 0,
                'code': Q - 1 if variant == 'A' else 0,
                'write_only': INT_SENTINEL}[fill]
        bad = words != want
        n = int(bad.sum())
        if n:
            at = int(torch.nonzero(bad)[0])
            raise guard.GuardError(
                '|'.join(names), 'back', at + 1, n,
                ' -- the owner\'s memory behind the view, after %s (tails %s;'
                ' word now 0x%08x)' % (what, variant,
                                       int(words[at]) & 0xffffffff))


def _bits(t):
    t = t.detach().clone()
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32)


def _session(kind, net, B, T, tails, variant, Q, check):
    """three training calls, a forward-only loss, score and predict_proba on
    views at (B, T); the tails checked after each; returns the results' bits"""
    rng = np.random.default_rng(1000 * B + T)
    out = []
    for i in range(3):
        inp = kind.inputs(rng, B, T)
        a, kw = kind.kwargs(net, inp, False)
        loss = net.loss(*a, **kw)
        torch.cuda.synchronize()
        what = 'training call %d' % i
        ws = net._ws[(B, T, True)]
        assert ws.capacity != ws.N and ws.T == T
        check(net, ws, net._step_path(ws, True))
        _check(tails, variant, Q, what)
        assert bool(torch.isfinite(loss)), (what, float(loss))
        out += [('loss%d' % i, _bits(loss.reshape(1))),
                ('grads%d' % i, _bits(net.grads))]
    inp = kind.inputs(rng, B, T)
    a, kw = kind.kwargs(net, inp, False)
    loss = net.loss(*a, backward=False, **kw)
    torch.cuda.synchronize()
    _check(tails, variant, Q, 'forward-only loss')
    fw = net._ws[(B, T, False)]
    assert fw.capacity != fw.N
    assert bool(torch.isfinite(loss))
    out += [('fwd_loss', _bits(loss.reshape(1))), ('logits', _bits(fw.logits))]
    s = net.score(*a, per_sample=True, **kw)
    torch.cuda.synchronize()
    _check(tails, variant, Q, 'score')
    # (a mixture head has no arg-max: correct is None there, and only there)
    assert (s.correct is None) == bool(net.mol_K)
    out += [('score_' + n, _bits(getattr(s, n)))
            for n in ('nll', 'count', 'correct', 'per_sample')
            if getattr(s, n) is not None]
    out.append(('score_logits', _bits(fw.logits)))
    pa, pkw = kind.proba_args(net, inp)
    p = net.predict_mixture(*pa, **pkw) if net.mol_K else \
        net.predict_proba(*pa, **pkw)
    torch.cuda.synchronize()
    _check(tails, variant, Q, 'predict_proba')
    assert bool(torch.isfinite(p).all())
    out.append(('proba', _bits(p)))
    net.check_device_errors()
    return out


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('name,kind,setup,check', KINDS,
                         ids=[k[0] for k in KINDS])
def test_view_calls_stay_inside_the_view(hip_lib, name, kind, setup, check, B):
    from wavenet import workspace
    net = kind.model(first=True, B=B)
    if setup:
        setup(net)
    assert net.use_launch_plans
    Q = net.Q
    no_tail = []
    for T in T_VIEWS:
        T_own = 2 * T + 37
        net._ws = {}
        rng = np.random.default_rng(T)
        a, kw = kind.kwargs(net, kind.inputs(rng, B, T_own), False)
        loss = net.loss(*a, **kw)                    # builds the owner
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss))
        owner = net._ws[(B, T_own, True)]
        assert owner.capacity == owner.N == B * T_own
        views = [workspace.get(net, B, T, True),
                 workspace.get(net, B, T, False)]
        for v in views:
            assert v.capacity == owner.N != v.N
            assert v.X.data_ptr() == owner.X.data_ptr()
        tails, none = _tails(owner, views)
        tailed = set(n for names, _, _ in tails for n in names)
        # the buffers the pass streams through all have one
        # (the slab scratch has one only where the split counts differ)
        for n in ('X', 'Z', 'SG', 'dZ', 'h1', 'h2', 'logits', 'q', 'dc1',
                  'dtotal', 'loss_parts', 'stack_flags'):
            assert n in tailed, (n, sorted(tailed))
        no_tail.append(set(none))
        results = []
        for variant in 'AB':
            _fill(tails, variant, Q)
            torch.cuda.synchronize()
            _check(tails, variant, Q, 'the fill')
            results.append(_session(kind, net, B, T, tails, variant, Q, check))
        owners = [w for w in net._ws.values() if w.capacity == w.N]
        assert owners == [owner]
        for (key, x), (key2, y) in zip(*results):
            assert key == key2
            if not torch.equal(x, y):
                bad = x != y
                raise guard.GuardError(
                    key, 'read', int(torch.nonzero(bad.reshape(-1))[0]),
                    int(bad.sum()),
                    ' -- %s B=%d T=%d: the result depends on what the owner '
                    'holds behind the view' % (name, B, T))
    if name not in _printed:
        _printed.add(name)
        never = set.intersection(*no_tail)
        print('%s: no tail at any length (size independent of T): %s; at '
              'some lengths only: %s'
              % (name, ', '.join(sorted(never)),
                 ', '.join(sorted(set.union(*no_tail) - never)) or 'none'))
