"""The training step's own orderings under a stall (tests/stall.py): the side
stream of the weight-gradient (TN) GEMMs with its fork and join, eagerly and
through recorded launch plans; launch plans keyed by the current stream; two
models on two streams at once.

Every sequence is three loss() calls with backward on one stream -- the eager,
the recording and the replaying leg of train_pass.run_pass -- with an Adam
step behind the first, so that the parameters change between record and
replay.  The reference is the same model, inputs and call sequence on the
default stream without any stall: loss, gradients and parameters bit for bit
(two such runs are compared first; a path that is not bit-reproducible would
fall back to check_grads alone and be listed in NOT_BITWISE: none is).  The
reference's gradients are held to the float64 oracle with test_gpu_model's
check_grads once per configuration.

Inputs are device tensors made before the stall: a host array would go up in
a pageable copy, which waits for the stream by design.  `lengths=` does
exactly that (ws.xent_mask.copy_ of a host array): for that case the
precondition is taken before the call.  Workspaces are reserved before the
stall (net.reserve): building one allocates, and the call that built one
under a stalled stream was seen to wait for the stall; with the workspace in
place the eager leg runs under the stall like the others.
The device is drained between two calls, so that every call meets a stall of
its own and an empty queue."""
import numpy as np
import pytest
import torch

import guard
import stall
from util import (TINY, MID, cfg_with, build_pair, tree_to_numpy,
                  oracle_grads_at_device_kinks)
from test_gpu_model import CASES as MODEL_CASES, check_grads

pytestmark = pytest.mark.gpu

NOT_BITWISE = ()                     # configurations compared by check_grads alone

# the stream-taking entries without a row in tests/test_gpu_guard_entries.py
# that this module runs through the host, each with the test that asserts
# (stall.spy) that the entry ran on the stalled stream
THROUGH_HOST = {
    'wn_stack_fwd_skip': 'test_non_default_current_stream[mid_S512]',
    'wn_stack_fwd': 'test_non_default_current_stream[tiny_ragged]',
    'wn_stack_bwd': 'test_non_default_current_stream[tiny_ragged]',
    'wn_stack_fwd_lc': 'test_non_default_current_stream_lc_and_lengths[lc]',
    'wn_stack_bwd_lc': 'test_non_default_current_stream_lc_and_lengths[lc]',
}

_BY_NAME = {c[0]: c for c in MODEL_CASES}
# 512 skip channels: the forward stack launch that also sums the skip
# convolutions (wn_stack_fwd_skip; tests/sat_ref.py's shape)
_BY_NAME['mid_S512'] = ('mid_S512', cfg_with(MID, batch_size=2,
                                             skip_channels=512), 150, False,
                        None)


def _cfg(name):
    """(cfg, T, gc, l2, model switches) of a configuration"""
    sw = {}
    if name == 'r64':
        sw = dict(overlap_tn=True)       # the blocked path's join
    _, cfg, T, gc, l2 = _BY_NAME[name]
    return cfg, T, gc, l2, sw


def _build(name, seed=0):
    cfg, T, gc, l2, sw = _cfg(name)
    net, var = build_pair(cfg, seed=seed)
    for k, v in sw.items():
        assert hasattr(net, k), k
        setattr(net, k, v)
    _reserve(net, T)
    return net


def _reserve(net, T):
    """both workspaces of the model, before any stall"""
    net.reserve(net.batch_size, T, training=True)
    net.reserve(net.batch_size, T, training=False)
    torch.cuda.synchronize()


BODY = guard._signed(guard.BODY32, 32)


def _bucket_mask(net, backward):
    """int32 words for the gradient bucket: the BODY pattern wherever one
    backward pass writes it, zeros in the alignment gaps between variables
    that no launch writes (a fresh bucket holds zeros there, and the
    optimizer walks the whole bucket)."""
    stall.body_fill(net.grads)
    backward()
    torch.cuda.synchronize()
    written = net.grads.view(torch.int32) != BODY
    assert int(written.sum()) > net.grads.numel() // 2
    return torch.where(written, BODY, 0).to(torch.int32)


_masks = {}


def _mask(name):
    if name not in _masks:
        cfg, T, gc, l2, _ = _cfg(name)
        net = _build(name)
        (a, ids), = _inputs(name, 1)
        _masks[name] = _bucket_mask(net, lambda: net.loss(a, ids, l2))
    return _masks[name]


def _inputs(name, calls, seed=7):
    """`calls` (audio, ids) pairs on the device"""
    cfg, T, gc, l2, _ = _cfg(name)
    B = cfg['batch_size']
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(calls):
        a = rng.uniform(-1, 1, (B, T)).astype(np.float32)
        ids = rng.integers(0, cfg['global_condition_cardinality'], B) \
            .astype(np.int32) if gc else None
        out.append((torch.from_numpy(a).cuda(),
                    None if ids is None else torch.from_numpy(ids).cuda()))
    torch.cuda.synchronize()
    return out


def _step(net, opt, i, a, ids, l2, fill=None, **kw):
    """call i of a sequence: loss with backward (an Adam step behind every
    third call, from the first), everything read back on the current stream"""
    if fill is not None:
        # a launch that ran early, on another stream, is not repaired by a
        # later one: the bucket holds the BODY pattern until the backward
        # pass on THIS stream writes it
        net.grads.view(torch.int32).copy_(fill)
    loss = net.loss(a, ids, l2, **kw)
    rec = {'loss': stall.bits(loss), 'grads': stall.bits(net.grads)}
    if i % 3 == 0:
        opt.minimize(loss)
        rec['params'] = stall.bits(net.params)
    return rec


def _optimizer():
    from wavenet.ops import AdamOptimizer
    return AdamOptimizer(1e-3)


def _assert_same(got, ref, what):
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert sorted(g) == sorted(r)
        for k in r:
            bad = g[k] != r[k]
            assert not bool(bad.any()), \
                '%s: %s of call %d differs from the default-stream run in ' \
                '%d of %d word(s)' % (what, k, i, int(bad.sum()), bad.numel())


def _assert_legs(net, stream, blocked=False, overlap=True):
    """eager, recording and replaying legs ran for this stream: a recorded
    plan per pass, keyed by the stream's handle"""
    ws = [w for w in net._ws.values() if w.training][0]
    mine = {k: v for k, v in ws.plans.items() if k[3] == stream.cuda_stream}
    tags = {k[0]: v for k, v in mine.items()}
    assert isinstance(tags.get('fwd'), list) and len(tags['fwd']) > 3, tags
    if not blocked:
        assert isinstance(tags.get('bwd'), list) and len(tags['bwd']) > 3
        assert any(n == 'py' for _, _, n, _ in tags['bwd']) == overlap
    path = [k[1] for k in mine if k[0] == 'fwd'][0]
    assert path.overlap_tn == overlap, path
    return ws


_ref = {}


def _reference(name, calls=3, fill=False):
    """The sequence on the default stream, twice (two fresh models): the
    records of the first run.  Once per configuration the gradients of its
    last call are held to the float64 oracle."""
    key = (name, calls, fill)
    if key in _ref:
        return _ref[key]
    cfg, T, gc, l2, _ = _cfg(name)
    x = _inputs(name, calls)
    mask = _mask(name) if fill else None
    runs = []
    for _ in range(2):
        net, opt = _build(name), _optimizer()
        runs.append([_step(net, opt, i, a, ids, l2, mask)
                     for i, (a, ids) in enumerate(x)])
        torch.cuda.synchronize()
    if name not in NOT_BITWISE:
        _assert_same(runs[1], runs[0], name + ' (two default-stream runs)')
    if not any(k[0] == name for k in _ref):
        # (the last call's gradients, at the parameters it ran with)
        a, ids = x[-1]
        var = tree_to_numpy(net.variables)
        _, ref_g, _, _ = oracle_grads_at_device_kinks(
            net, cfg, var, a.cpu().numpy(),
            None if ids is None else ids.cpu().numpy(), l2)
        check_grads(net, ref_g)
    _ref[key] = runs[0]
    return runs[0]


STEP_CASES = ['tiny_ragged', 'gc', 'r64']


def _stalled_sequence(name, which):
    """The three-call sequence on the default stream with `which` ('side' or
    'main') stalled before each call."""
    cfg, T, gc, l2, _ = _cfg(name)
    ref = _reference(name)
    x = _inputs(name, 3)
    main = torch.cuda.default_stream()
    side = stall.concurrent_stream(main)

    def attempt(ms):
        net, opt = _build(name), _optimizer()
        net._side = side
        torch.cuda.synchronize()
        got, held = [], []
        for i, (a, ids) in enumerate(x):
            st = stall.Stall(side if which == 'side' else main, ms)
            got.append(_step(net, opt, i, a, ids, l2))
            # nothing in the call waits for the device: the whole step is
            # queued behind (or beside) the stall
            held.append(st.pending())
            torch.cuda.synchronize()
        assert net._side is side
        _assert_legs(net, main, blocked=name == 'r64')
        _assert_same(got, ref, '%s, %s stream stalled %d ms' % (name, which, ms))
        net.check_device_errors()
        return all(held)
    stall.first_rung(attempt)


@pytest.mark.parametrize('name', STEP_CASES)
def test_side_stream_late(hip_lib, name):
    """The side stream stalled before each call: when its TN GEMMs read, the
    main stream has run the dZ GEMM, the backward stack and everything else up
    to the join.  An input of theirs that the main stream rewrites before the
    join, or a slab reduction that does not wait for the join, gives other
    post1 / post2 / skip gradients."""
    _stalled_sequence(name, 'side')


@pytest.mark.parametrize('name', STEP_CASES)
def test_main_stream_late(hip_lib, name):
    """The main stream stalled before each call: the side stream is idle and
    would run the TN GEMMs at once, before dc1 / dtotal exist, if it did not
    wait for the fork."""
    _stalled_sequence(name, 'main')


# ---- a current stream that is not the default stream -----------------------
def _lc_case():
    import test_gpu_local_condition as t
    biases, gc, Lc, B, T, dil = min(t.CASES, key=lambda c: c[3] * c[4])
    codes, lc = t._inputs(B, T, 64, Lc, seed=B + Lc)
    ids = None if gc is None else (np.arange(B) % gc).astype(np.int32)

    def build():
        net = t._model(B, Lc, dil, biases=biases, gc=gc, seed=len(dil))
        _reserve(net, T)
        return net
    kw = dict(local_condition_batch=torch.from_numpy(lc).cuda())
    return build, torch.from_numpy(codes).cuda(), \
        None if ids is None else torch.from_numpy(ids).cuda(), kw


def _masked_case():
    import test_gpu_masked_loss as t
    name, mkw, T, lengths, rows, audio = min(
        (c for c in t.CASES if not c[1].get('Lc') and c[4] is not None),
        key=lambda c: len(c[3]) * c[2])
    B = len(lengths)
    gc = mkw.get('gc')
    ids = None if gc is None else (np.arange(B) % gc).astype(np.int32)

    def build():
        net = t._model(B, seed=T, **mkw)
        _reserve(net, T)
        return net
    codes = t._codes(B, T, mkw.get('Q', 256), T)
    return build, torch.from_numpy(codes).cuda(), \
        None if ids is None else torch.from_numpy(ids).cuda(), \
        dict(lengths=np.asarray(lengths))


def _codes_sequence(net, opt, codes, ids, kw, mask, before=None, after=None):
    """three loss_from_codes calls (the codes rotated by the call's number),
    the bucket pre-filled"""
    out = []
    qs = [torch.roll(codes, i, 1).contiguous() for i in range(3)]
    torch.cuda.synchronize()
    for i, q in enumerate(qs):
        if before:
            before(i)
        net.grads.view(torch.int32).copy_(mask)
        loss = net.loss_from_codes(q, ids, **kw)
        rec = {'loss': stall.bits(loss), 'grads': stall.bits(net.grads)}
        if after:
            after(i)
        torch.cuda.synchronize()
        if i == 0:
            opt.minimize(loss)
            rec['params'] = stall.bits(net.params)
        out.append(rec)
    return out


EXPECT = {
    'tiny_ragged': {'wn_stack_fwd', 'wn_stack_bwd', 'wn_gemm_tn'},
    'mid_S512': {'wn_stack_fwd_skip', 'wn_stack_bwd'},
    'gc': {'wn_gc_bias', 'wn_gc_grad', 'wn_stack_bwd'},
    'lc': {'wn_stack_fwd_lc', 'wn_stack_bwd_lc'},
    'masked': {'wn_xent_masked'},
}


@pytest.mark.parametrize('name', ['tiny_ragged', 'mid_S512', 'gc'])
def test_non_default_current_stream(hip_lib, name):
    """The sequence under stalled stream s1, then s2, then s1 again: two plan
    sets keyed by the stream, the third run replays the first's.  Then the
    forward-only loss and score() under s2.  Every stream-taking entry was
    given the current stream or the side stream, never another."""
    cfg, T, gc, l2, _ = _cfg(name)
    ref = _reference(name, calls=9, fill=True)
    x, mask = _inputs(name, 9), _mask(name)
    # forward-only loss and the score of the last batch at the final
    # parameters, on the default stream
    rnet, ropt = _build(name), _optimizer()
    for i, (a, ids) in enumerate(x):
        _step(rnet, ropt, i, a, ids, l2, mask)
    a, ids = x[-1]
    ref_fwd = stall.bits(rnet.loss(a, ids, l2, backward=False))
    sc = rnet.score(a, ids)
    ref_score = [stall.bits(t) for t in (sc.nll, sc.count, sc.correct)]
    torch.cuda.synchronize()
    s1 = stall.concurrent_stream(torch.cuda.default_stream())
    s2 = stall.concurrent_stream(torch.cuda.default_stream(), s1)

    def attempt(ms):
        net, opt = _build(name), _optimizer()
        torch.cuda.synchronize()
        got, held = [], []
        with stall.spy(hip_lib) as seen:
            for turn, s in enumerate((s1, s2, s1)):
                with torch.cuda.stream(s):
                    for i in range(3 * turn, 3 * turn + 3):
                        st = stall.Stall(s, ms)
                        got.append(_step(net, opt, i, *x[i], l2, mask))
                        held.append(st.pending())
                        s.synchronize()
                s.synchronize()
            with torch.cuda.stream(s2):
                st = stall.Stall(s2, ms)
                fwd = stall.bits(net.loss(a, ids, l2, backward=False))
                sc = net.score(a, ids)
                score = [stall.bits(t) for t in (sc.nll, sc.count, sc.correct)]
                held.append(st.pending())
            torch.cuda.synchronize()
        print('%s ran: %s' % (name, ' '.join(sorted(seen))))
        _assert_same(got, ref, '%s, current stream stalled %d ms' % (name, ms))
        assert torch.equal(fwd, ref_fwd)
        for g, r in zip(score, ref_score):
            assert torch.equal(g, r)
        ws = _assert_legs(net, s1)
        _assert_legs(net, s2)
        assert len(set(k[3] for k in ws.plans)) == 2
        ok = {s1.cuda_stream, s2.cuda_stream, net._side.cuda_stream}
        assert torch.cuda.default_stream().cuda_stream not in ok
        for entry, handles in seen.items():
            assert handles <= ok, (entry, handles, ok)
        assert EXPECT[name] <= set(seen), (EXPECT[name] - set(seen))
        assert seen['wn_gemm_tn'] == {net._side.cuda_stream}
        # every variable's gradient was written: no word of the pre-fill left
        for n, g in net.named_variables(net.gradients):
            assert bool(torch.isfinite(g).all()), n
        net.check_device_errors()
        return all(held)
    stall.first_rung(attempt)


@pytest.mark.parametrize('name', ['lc', 'masked'])
def test_non_default_current_stream_lc_and_lengths(hip_lib, name):
    """Local conditioning (the _lc stack launches) and `lengths=` under a
    stalled stream that is not the default stream.  `lengths=` stages a host
    array with a pageable copy, which waits for the stream by design: its
    precondition is taken before each call."""
    build, codes, ids, kw = _lc_case() if name == 'lc' else _masked_case()
    torch.cuda.synchronize()
    net = build()
    mask = _bucket_mask(net, lambda: net.loss_from_codes(codes, ids, **kw))
    refs = []
    for _ in range(2):
        refs.append(_codes_sequence(build(), _optimizer(), codes, ids, kw,
                                    mask))
        torch.cuda.synchronize()
    _assert_same(refs[1], refs[0], name + ' (two default-stream runs)')
    s = stall.concurrent_stream(torch.cuda.default_stream())

    def attempt(ms):
        net, opt = build(), _optimizer()
        torch.cuda.synchronize()
        held, st = [], []

        def before(i):
            st.append(stall.Stall(s, ms))
            if name == 'masked':
                held.append(st[-1].pending())

        def after(i):
            if name != 'masked':
                held.append(st[-1].pending())
        with torch.cuda.stream(s), stall.spy(hip_lib) as seen:
            got = _codes_sequence(net, opt, codes, ids, kw, mask, before,
                                  after)
        print('%s ran: %s' % (name, ' '.join(sorted(seen))))
        torch.cuda.synchronize()
        _assert_same(got, refs[0], '%s, stalled %d ms' % (name, ms))
        _assert_legs(net, s)
        ok = {s.cuda_stream, net._side.cuda_stream}
        for entry, handles in seen.items():
            assert handles <= ok, (entry, handles, ok)
        assert EXPECT[name] <= set(seen), (EXPECT[name] - set(seen))
        for n, g in net.named_variables(net.gradients):
            assert bool(torch.isfinite(g).all()), n
        net.check_device_errors()
        return all(held)
    stall.first_rung(attempt)


# ---- two models, two streams ------------------------------------------------
def test_two_models_on_two_streams(hip_lib):
    """The header's re-entrancy claim: two independently seeded TINY models
    run one step each, model 0 under s1 and model 1 under s2, their calls
    queued in turn, with s1 stalled, then s2, then both (the two persistent
    stack launches are then in flight at once: B * ceil(T / 32) = 8 tiles per
    model, both grids resident whatever the schedule).  Each model's loss and
    gradients equal its own serial default-stream result.  The two models
    share one side stream, so that the test holds four streams."""
    cfg = cfg_with(TINY, batch_size=2)
    T = 100
    assert cfg['batch_size'] * ((T + 31) // 32) <= 8
    rng = np.random.default_rng(3)
    audio = [torch.from_numpy(rng.uniform(-1, 1, (2, T)).astype(np.float32))
             .cuda() for _ in range(2)]

    def build():
        nets = [build_pair(cfg, seed=k)[0] for k in range(2)]
        for net in nets:
            _reserve(net, T)
        return nets
    probe = build()[0]
    mask = _bucket_mask(probe, lambda: probe.loss(audio[0]))
    ref = []
    for net, a in zip(build(), audio):
        net.grads.view(torch.int32).copy_(mask)
        loss = net.loss(a)
        ref.append({'loss': stall.bits(loss), 'grads': stall.bits(net.grads)})
        torch.cuda.synchronize()
    assert not torch.equal(ref[0]['grads'], ref[1]['grads'])
    s1 = stall.concurrent_stream(torch.cuda.default_stream())
    s2 = stall.concurrent_stream(torch.cuda.default_stream(), s1)
    side = torch.cuda.Stream()

    def attempt(ms):
        ok = True
        for stalled in ((s1,), (s2,), (s1, s2)):
            nets = build()
            for net in nets:
                net._side = side
                net.grads.view(torch.int32).copy_(mask)
            torch.cuda.synchronize()
            sts = [stall.Stall(s, ms) for s in stalled]
            got = []
            for net, a, s in zip(nets, audio, (s1, s2)):
                with torch.cuda.stream(s):
                    loss = net.loss(a)
                    got.append({'loss': stall.bits(loss),
                                'grads': stall.bits(net.grads)})
            ok = ok and all(st.pending() for st in sts)
            torch.cuda.synchronize()
            for k in range(2):
                _assert_same([got[k]], [ref[k]],
                             'model %d, %d stream(s) stalled %d ms'
                             % (k, len(stalled), ms))
                nets[k].check_device_errors()
                ws = list(nets[k]._ws.values())[0]
                assert any(key[1].bwd == 'stack' and key[1].overlap_tn
                           for key in ws.plans), list(ws.plans)
        return ok
    stall.first_rung(attempt)
