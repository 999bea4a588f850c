"""Models with a mixture-of-logistics head, with and without global and local
conditioning, end to end against the float64 network of tests/mol_ref.py:
the loss and EVERY variable's gradient within the project's bound (2e-5 of each variable's largest entry), the score / loss
relations, predict_mixture against the float64 network's last row, and a few
Adam steps that lower the loss."""
import numpy as np
import pytest
import torch

import lc_ref
import mol_cases as MC
import mol_ref as R
from util import synth_audio

pytestmark = pytest.mark.gpu

TOL = 2e-5     # of each variable's largest entry (the project's bar)
DIL = [1, 2, 4, 1, 2]
B, T, S, LC = 2, 200, 32, 5
SCALES = (2, 4)


def _model(K, ch=16, ifw=2, biases=False, gc=None, lc=None, seed=0, lsm=-14.0):
    from wavenet import WaveNetModel
    kw = {}
    if gc:
        kw.update(global_condition_channels=gc, global_condition_cardinality=gc)
    if lc:
        kw['local_condition_channels'] = LC
    if lc == 'up':
        kw.update(local_condition_upsample_scales=SCALES,
                  local_condition_context=1)
    kw.update(output_mixture=K, mixture_log_scale_min=lsm)
    net = WaveNetModel(B, DIL, 2, ch, ch, S, quantization_channels=64,
                       use_biases=biases, scalar_input=True,
                       initial_filter_width=ifw, seed=seed, **kw)
    g = torch.Generator().manual_seed(seed + 11)

    def rnd(v, s):
        v.copy_((s * torch.randn(v.shape, generator=g,
                                 dtype=torch.float64)).float())
    with torch.no_grad():
        for n, v in net.named_variables():
            last = n.split('/')[-1]
            if '/lc_upsample/' in n or '/lc_context/' in n:
                rnd(v, 0.5)
            elif 'bias' in last:
                rnd(v, 0.1)
            elif last.startswith('lc_'):
                rnd(v, 0.3)
        if biases:
            # scales round e^-2 of full scale: narrow enough that the bins
            # matter, wide enough that float32 logits still place the mean
            Kp = net.mol_Kp
            net.variables['postprocessing']['postprocess2_bias'][
                2 * Kp:2 * Kp + K] -= 2.0
    return net


def _lc_input(lc, seed, B=B, T=T):
    rng = np.random.default_rng(seed)
    if lc == 'rows':
        return rng.standard_normal((B, T, LC)).astype(np.float32)
    if lc == 'up':
        F = (T - 1) // int(np.prod(SCALES)) + 1
        return rng.standard_normal((B, F, LC)).astype(np.float32)
    return None


def _reference(net, audio, K, lc, lcin, ids, lengths, history, grads=True):
    """The float64 network on what the device network read (audio [B, T],
    any B)."""
    from wavenet import mol
    B, T = np.shape(audio)
    n = np.full(B, T) if lengths is None else np.asarray(lengths)
    h = np.zeros(B, np.int64) if history is None else np.asarray(history)
    den = float(B * T) if lengths is None and history is None else \
        float((n - h).sum())
    lv, x = mol.levels_reference(audio, lengths)
    head = (K, net.mol_log_scale_min)
    tgt = R.targets(lv, lengths, history)
    masks = lc_ref.device_relu_masks(net, B, T) if grads else None
    return R.network(lc_ref.model_tree(net), DIL, x, tgt, den, head, lc=lcin,
                     scales=SCALES if lc == 'up' else None, gc_ids=ids,
                     use_biases=net.use_biases, relu_masks=masks, grads=grads)


# (id, K, channels, initial_filter_width, biases, gc, lc,
#  lengths, history)
CASES = [
    ('k4_plain', 4, 16, 2, False, None, None, None, None),
    ('k10_ifw32_bias_gc', 10, 32, 32, True, 3, None, None, None),
    ('k4_lc_rows_gc', 4, 16, 32, True, 2, 'rows', None, None),
    ('k10_lc_up', 10, 32, 2, True, None, 'up', None, None),
    ('k10_lc_up_ragged_hist', 10, 16, 32, True, 3, 'up', [200, 131], [0, 17]),
    ('k4_ragged', 4, 32, 2, False, None, None, [150, 200], None),
    ('k1_hist', 1, 16, 2, True, None, None, None, [40, 0]),
]


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_loss_and_every_gradient_match_float64(hip_lib, case):
    name, K, ch, ifw, biases, gc, lc, lengths, history = case
    net = _model(K, ch, ifw, biases, gc, lc, seed=len(name))
    audio = synth_audio(B, T, seed=7 + len(name))
    lcin = _lc_input(lc, 3)
    ids = None if gc is None else np.arange(B) % gc
    kw = dict(lengths=lengths, history=history)
    if lc:
        kw['local_condition_batch'] = lcin
    for _ in range(3):               # eager, recorded, replayed
        loss = float(net.loss(audio, ids, **kw))
    torch.cuda.synchronize()
    ref_loss, ref_g, _, ref_rows = _reference(net, audio, K, lc, lcin, ids,
                                              lengths, history)
    print('%s: loss %.7f, float64 %.7f' % (name, loss, ref_loss))
    assert abs(loss - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
    got = dict(lc_ref.flatten(lc_ref.model_tree(net, grads=True)))
    ref = dict(lc_ref.flatten(ref_g))
    assert sorted(got) == sorted(ref)
    bad, worst = [], 0.0
    for k in sorted(ref):
        scale = np.abs(ref[k]).max()
        err = np.abs(got[k] - ref[k]).max()
        # (the last layer's dense weights feed nothing: exact zeros)
        worst = max(worst, err / max(scale, 1e-30))
        if not err <= TOL * max(scale, 1e-30):
            bad.append((k, float(err), float(scale)))
    print('%s: worst gradient error %.3g of the variable\'s largest entry'
          % (name, worst))
    assert not bad, bad[:6]
    # score: the relations of WaveNetModel.score's docstring
    sc = net.score(audio, ids, per_sample=True,
                   **{k: v for k, v in kw.items()})
    fwd = float(net.loss(audio, ids, backward=False, **kw))
    n = np.full(B, T) if lengths is None else np.asarray(lengths)
    h = np.zeros(B, np.int64) if history is None else np.asarray(history)
    den = B * T if lengths is None and history is None else (n - h).sum()
    nll = sc.nll.cpu().numpy()
    assert abs(fwd - nll.sum() / den) <= 2e-6 * max(1.0, abs(fwd))
    assert abs(fwd - loss) <= 2e-6 * max(1.0, abs(loss))
    assert sc.count.cpu().numpy().tolist() == (n - np.maximum(h, 1)).tolist()
    rows = sc.per_sample.cpu().numpy()
    assert np.abs(rows - ref_rows).max() <= 2e-5 * max(1.0, np.abs(ref_rows).max())
    assert (rows[ref_rows == 0] == 0).all()
    assert sc.correct is None


@pytest.mark.parametrize('K,ifw,lc,gc', [(4, 2, None, None), (10, 32, 'rows', 2)])
def test_predict_mixture_is_the_float64_last_row(hip_lib, K, ifw, lc, gc):
    """Held to the kernel test's yardstick: four times the larger of a
    float32 restatement's own error (the same torch network in float32) and
    one float32 ulp of the block's largest entry."""
    from wavenet import WaveNetModel, mol
    net = _model(K, 16, ifw, True, gc, lc, seed=K)
    one = WaveNetModel(1, DIL, 2, 16, 16, S, quantization_channels=64,
                       use_biases=True, scalar_input=True,
                       initial_filter_width=ifw, output_mixture=K,
                       global_condition_channels=gc,
                       global_condition_cardinality=gc,
                       local_condition_channels=LC if lc else None)
    one.load_state_dict(net.state_dict())
    audio = synth_audio(1, 77, seed=5)[0]
    rows = None if lc is None else \
        np.random.default_rng(2).standard_normal((77, LC)).astype(np.float32)
    ids = None if gc is None else [1]
    got = one.predict_mixture(audio, ids, local_condition=rows).cpu().numpy()
    assert got.shape == (3, K) and np.isfinite(got).all()
    _, x = mol.levels_reference(audio[None])
    var = lc_ref.model_tree(one)
    outs = {}
    for dt in (torch.float64, torch.float32):
        v = lc_ref._to_torch(var)
        cast = lambda t: t.detach().to(dt)
        tree = {k: ([{kk: cast(vv) for kk, vv in c.items()} for c in val]
                    if isinstance(val, list) else
                    {kk: cast(vv) for kk, vv in val.items()})
                for k, val in v.items()}
        with torch.no_grad():
            raw = R.forward(tree, DIL, torch.as_tensor(x).to(dt),
                            None if rows is None else
                            torch.as_tensor(rows[None]).to(dt), ids, True)
        outs[dt] = R.params(raw[0, -1].double().numpy(), K,
                            one.mol_log_scale_min)
    r64, r32 = outs[torch.float64], outs[torch.float32]
    for blk in range(3):
        own = np.abs(r32[blk] - r64[blk]).max()
        bound = 4.0 * max(own, float(MC.ulp32(np.abs(r64[blk]).max())))
        err = np.abs(got[blk] - r64[blk]).max()
        print('predict_mixture K=%d block %d: error / bound %.3f'
              % (K, blk, err / bound))
        assert err <= bound, (blk, err, bound)


def test_adam_steps_lower_the_loss(hip_lib):
    from wavenet import optimizer_factory
    net = _model(10, 32, 32, True, 2, 'rows', seed=3)
    audio = synth_audio(B, T, seed=9)
    lcin = _lc_input('rows', 4)
    opt = optimizer_factory['adam'](learning_rate=1e-3, momentum=0.9)
    losses = []
    for _ in range(30):
        loss = net.loss(audio, [0, 1], local_condition_batch=lcin)
        opt.minimize(loss)
        losses.append(float(loss))
    assert np.isfinite(losses).all()
    assert losses[-1] < losses[0] - 0.05, (losses[0], losses[-1])


# ---- launch-plan replay, ragged batches, views --------------------------------
def _bits(x):
    x = x.detach().reshape(-1)
    return x.view(torch.int64 if x.element_size() == 8 else torch.int32)


def _replayed(ws, tag):
    """a recorded launch plan of pass `tag` exists: the next call replays"""
    return ws is not None and any(k[0] == tag and isinstance(p, list)
                                  for k, p in ws.plans.items())


def _twin(net, *args, **kw):
    """A second model (_model's arguments) with net's parameters."""
    other = _model(*args, **kw)
    with torch.no_grad():
        other.params.copy_(net.params)
    return other


def _new_inputs(i, gc, Bq=B):
    """audio, GC ids and LC rows that differ from call to call"""
    audio = np.roll(synth_audio(Bq, T, seed=30 + i), 37 * i, 1) * \
        np.float32(1.0 - 0.12 * i)
    return audio, (np.arange(Bq) + i) % gc, _lc_input('rows', 50 + i, Bq)


def _hold_loss_to_float64(what, net, loss, audio, K, lcin, ids, lengths,
                          history):
    ref_loss, ref_g, _, _ = _reference(net, audio, K, 'rows', lcin, ids,
                                       lengths, history)
    assert abs(loss - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), \
        (what, loss, ref_loss)
    got = dict(lc_ref.flatten(lc_ref.model_tree(net, grads=True)))
    ref = dict(lc_ref.flatten(ref_g))
    assert sorted(got) == sorted(ref)
    bad, worst = [], 0.0
    for k in sorted(ref):
        scale = np.abs(ref[k]).max()
        err = np.abs(got[k] - ref[k]).max()
        worst = max(worst, err / max(scale, 1e-30))
        if not err <= TOL * max(scale, 1e-30):
            bad.append((k, float(err), float(scale)))
    print('%s: loss %.7f, float64 %.7f; worst gradient error %.3g of the '
          'variable\'s largest entry' % (what, loss, ref_loss, worst))
    assert not bad, (what, bad[:6])


def _hold_score_to_float64(what, net, sc, audio, K, lcin, ids, lengths,
                           history):
    Bq = audio.shape[0]
    _, _, _, ref_rows = _reference(net, audio, K, 'rows', lcin, ids, lengths,
                                   history, grads=False)
    n = np.full(Bq, T) if lengths is None else np.asarray(lengths)
    h = np.zeros(Bq, np.int64) if history is None else np.asarray(history)
    rows = sc.per_sample.cpu().numpy()
    assert rows.shape == ref_rows.shape == (Bq, T)
    err = np.abs(rows - ref_rows).max()
    print('%s: per-row error %.3g of max(1, largest row)'
          % (what, err / max(1.0, np.abs(ref_rows).max())))
    assert err <= 2e-5 * max(1.0, np.abs(ref_rows).max()), what
    assert (rows[ref_rows == 0] == 0).all(), what
    assert sc.count.cpu().numpy().tolist() == (n - np.maximum(h, 1)).tolist()
    # (a clip's nll: the float64 sum of its rows, each within the row bound)
    nll = sc.nll.cpu().numpy()
    assert (np.abs(nll - ref_rows.sum(1)) <= (n - np.maximum(h, 1)) * 2e-5 *
            max(1.0, np.abs(ref_rows).max())).all(), what
    # (... of the float32 rows it returns, in another order: T float64
    # roundings at the most)
    assert np.abs(nll - rows.astype(np.float64).sum(1)).max() <= \
        T * 2.0 ** -52 * max(1.0, np.abs(nll).max()), what
    assert sc.correct is None


def test_replay_tracks_new_inputs(hip_lib):
    """Five loss calls on one workspace -- eager, recorded, replayed three
    times -- and three score calls on the forward-only one, every call with
    new audio, GC ids and LC rows and other lengths and history: each against
    float64 and, bit for bit, against a model without launch plans.  What a
    replay could read stale: the levels and centres wn_mol_quantize writes
    outside the plan, the mask and history words, the ids, the LC rows."""
    K, gc = 10, 3
    args = (K, 32, 32, True, gc, 'rows')
    net = _model(*args, seed=21)
    plain = _twin(net, *args, seed=21)
    plain.use_launch_plans = False
    assert net.use_launch_plans
    calls = [(None, None), ([200, 131], [0, 17]), (None, [40, 0]),
             ([77, 200], None), (None, None)]
    seen = []
    for i, (lengths, history) in enumerate(calls):
        audio, ids, lcin = _new_inputs(i, gc)
        kw = dict(lengths=lengths, history=history,
                  local_condition_batch=lcin)
        ws = net._ws.get((B, T, True))
        for tag in ('fwd', 'bwd'):
            assert _replayed(ws, tag) == (i >= 2), (i, tag)
        out = [m.loss(audio, ids, **kw) for m in (net, plain)]
        torch.cuda.synchronize()
        assert torch.equal(_bits(out[0]), _bits(out[1])), \
            (i, float(out[0]), float(out[1]))
        assert torch.equal(net.grads, plain.grads), i
        assert ws is None or ws is net._ws[(B, T, True)]
        assert not plain._ws[(B, T, True)].plans
        _hold_loss_to_float64('replay, loss call %d' % (i + 1), net,
                              float(out[0]), audio, K, lcin, ids, lengths,
                              history)
        seen.append(float(out[0]))
    assert len(set(seen)) == len(seen)           # (the inputs did change)
    for i, (lengths, history) in enumerate([([131, 200], [17, 0]),
                                            (None, None),
                                            ([200, 9], [150, 8])]):
        audio, ids, lcin = _new_inputs(7 + i, gc)
        kw = dict(lengths=lengths, history=history,
                  local_condition_batch=lcin, per_sample=True)
        ws = net._ws.get((B, T, False))
        assert _replayed(ws, 'fwd') == (i >= 2), i
        out = [m.score(audio, ids, **kw) for m in (net, plain)]
        torch.cuda.synchronize()
        for name in ('nll', 'count', 'per_sample'):
            assert torch.equal(_bits(getattr(out[0], name)),
                               _bits(getattr(out[1], name))), (i, name)
        assert ws is None or ws is net._ws[(B, T, False)]
        _hold_score_to_float64('replay, score call %d' % (i + 1), net, out[0],
                               audio, K, lcin, ids, lengths, history)
    net.check_device_errors()


def test_ragged_batches_single_clips_and_predict_on_a_view(hip_lib):
    """score() of [B', T] with B' = 1 and 3 on a model built for batches of
    two, with lengths and history: against float64, and bit for bit against
    the same clips scored one at a time.  Then predict_mixture, on its own
    workspace and -- after a training step at a longer T -- on a view of the
    training owner, bit for bit against a fresh model's."""
    from wavenet import optimizer_factory
    K, gc = 10, 3
    args = (K, 16, 32, True, gc, 'rows')
    net = _model(*args, seed=8)
    assert net.batch_size == 2
    for Bq, lengths, history in ((1, [150], [33]),
                                 (3, [200, 131, 64], [0, 17, 63])):
        audio, ids, lcin = _new_inputs(Bq, gc, Bq)
        sc = net.score(audio, ids, lengths=lengths, history=history,
                       local_condition_batch=lcin, per_sample=True)
        torch.cuda.synchronize()
        assert net._ws[(Bq, T, False)].B == Bq
        assert sc.nll.shape == (Bq,) and sc.per_sample.shape == (Bq, T)
        _hold_score_to_float64("ragged B' = %d" % Bq, net, sc, audio, K,
                               lcin, ids, lengths, history)
        for b in range(Bq):
            one = net.score(audio[b:b + 1], ids[b:b + 1],
                            lengths=lengths[b:b + 1],
                            history=history[b:b + 1],
                            local_condition_batch=lcin[b:b + 1],
                            per_sample=True)
            for name in ('nll', 'count', 'per_sample'):
                assert torch.equal(_bits(getattr(sc, name)[b]),
                                   _bits(getattr(one, name))), (Bq, b, name)

    def predict(m, Tp, seed):
        rng = np.random.default_rng(seed)
        rows = rng.standard_normal((B, Tp, LC)).astype(np.float32)
        out = m.predict_mixture(synth_audio(B, Tp, seed=seed), [2, 1],
                                local_condition=rows)
        torch.cuda.synchronize()
        assert out.shape == (3, K) and bool(torch.isfinite(out).all())
        return out

    got = predict(net, 77, 1)
    assert torch.equal(_bits(got), _bits(predict(_twin(net, *args), 77, 1)))
    audio, ids, lcin = _new_inputs(0, gc)
    audio = np.concatenate([audio, audio[:, :100]], 1)          # T = 300
    lcin = np.concatenate([lcin, lcin[:, :100]], 1)
    opt = optimizer_factory['adam'](learning_rate=1e-3, momentum=0.9)
    opt.minimize(net.loss(audio, ids, local_condition_batch=lcin))
    got = predict(net, 150, 2)
    view, owner = net._ws[(B, 150, False)], net._ws[(B, 300, True)]
    assert view.capacity == owner.N != view.N
    assert view.logits.data_ptr() == owner.logits.data_ptr()
    assert torch.equal(_bits(got), _bits(predict(_twin(net, *args), 150, 2)))
    net.check_device_errors()
