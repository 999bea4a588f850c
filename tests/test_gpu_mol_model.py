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


def _lc_input(lc, seed):
    rng = np.random.default_rng(seed)
    if lc == 'rows':
        return rng.standard_normal((B, T, LC)).astype(np.float32)
    if lc == 'up':
        F = (T - 1) // int(np.prod(SCALES)) + 1
        return rng.standard_normal((B, F, LC)).astype(np.float32)
    return None


def _reference(net, audio, K, lc, lcin, ids, lengths, history, grads=True):
    """The float64 network on what the device network read."""
    from wavenet import mol
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
