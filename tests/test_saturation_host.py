"""The saturated cases of tests/test_gpu_saturation.py on the CPU: every case
reaches the regime it is there for, and tests/sat_ref.py's one-block
restatements reproduce the oracle when chained.

What the planted biases (sat_ref.PLANTS) force, in the float64 oracle:
  layer 1 gate_bias[0] = -120   sigmoid < 1e-45: exactly 0 in float32
  layer 1 gate_bias[1] = +120   sigmoid exactly 1
  layer 2 filter_bias[2] = -60  tanh -1
  layer 2 filter_bias[3] = +60  tanh +1
  layer 3 gate_bias[4] = -60    sigmoid ~ 1e-26, inside (1e-30, 1e-22) where the
                                device's `+ 1e-30f` guard changes tanh = z / s
"""
import numpy as np
import pytest

import sat_ref as S
from util import O, flat_named

_ALL = [(n, g) for n, c in S.CASES.items() for g in c[2]]


def _cache(name, gain):
    """float64 forward cache of a case: the oracle's where it can evaluate the
    model (no local conditioning), sat_ref.forward_chain's otherwise."""
    cfg = S.CASES[name][0]
    var = S.saturated_variables(cfg, gain)
    codes, audio, lc = S.case_inputs(name)
    if lc is not None:
        return S.forward_chain(cfg, var, codes, lc, np.float64)
    enc = O.one_hot(codes, cfg['quantization_channels'], np.float64)
    _, c = O.network_forward(cfg, var, enc, keep=True)
    return c


@pytest.mark.parametrize('name,gain', _ALL, ids=['%s-g%g' % a for a in _ALL])
def test_case_reaches_the_saturated_regime(name, gain):
    cov = S.coverage(_cache(name, gain)['layers'])
    print(name, gain, cov)
    S.assert_coverage(cov, (name, gain))


def test_plants_force_what_they_are_there_for():
    c = _cache('mid', 3.0)['layers']
    assert (c[1]['sig'][..., 0] < 1e-45).all()
    assert (c[1]['sig'][..., 1] == 1.0).all()
    assert (c[2]['tanh'][..., 2] == -1.0).all() and (c[2]['tanh'][..., 3] == 1.0).all()
    s = c[3]['sig'][..., 4]
    assert ((s > 1e-30) & (s < 1e-22)).any()
    # float32: exactly 0, and the oracle's own float32 evaluation agrees
    assert (c[1]['sig'][..., 0].astype(np.float32) == 0).all()


def test_nobias_model_gets_gain_6_and_no_plants():
    cfg = S.cfg_with(S.MID, batch_size=1, use_biases=False)
    a = S.saturated_variables(cfg, 3.0)
    b = O.create_variables(cfg, seed=0, dtype=np.float64)
    for x, y in zip(a['dilated_stack'], b['dilated_stack']):
        assert np.array_equal(x['filter'], 6.0 * y['filter'])
        assert np.array_equal(x['gate'], 6.0 * y['gate'])
        assert np.array_equal(x['dense'], y['dense']) and 'gate_bias' not in x


@pytest.mark.parametrize('name', ['mid', 'mid_k3', 'r64', 'tiny', 'mid_T20'])
def test_chained_restatement_reproduces_the_oracle(name):
    """layer_forward / layer_backward in float64, chained over the layers,
    against oracle.loss_and_grads' per-layer cache and gradients (1e-12 of
    each tensor's largest entry: the same operations in float64)."""
    cfg = S.CASES[name][0]
    var = S.saturated_variables(cfg, 3.0)
    codes, audio, _ = S.case_inputs(name)
    B, T = codes.shape
    K, dil, L = cfg['filter_width'], cfg['dilations'], len(cfg['dilations'])
    loss, g, c = O.loss_and_grads(cfg, var, audio, dtype=np.float64,
                                  return_cache=True)

    def same(a, b, what):
        assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max()), what
    mine = S.forward_chain(cfg, var, codes, None, np.float64)
    for l in range(L):
        for k in ('x', 'tanh', 'sig', 'z'):
            same(mine['layers'][l][k], c['layers'][l][k], (l, k))
    same(mine['total'], c['total'], 'total')
    same(mine['logits'], c['logits'], 'logits')
    # dtotal as loss_and_grads forms it, then dZ_l = dtotal Ws_l^T per layer
    pp = var['postprocessing']
    dlogits = (np.exp(c['logp']) - c['shifted']) / (B * T)
    dc1 = (dlogits @ pp['postprocess2'][0].T) * (c['c1'] > 0)
    dtotal = (dc1 @ pp['postprocess1'][0].T) * (c['total'] > 0)
    dx = None
    for l in reversed(range(L)):
        blk = S.block_of(var, l, dil, K)
        x = c['layers'][l]['x']
        dZ = dtotal @ var['dilated_stack'][l]['skip'][0].T
        out = S.layer_backward(x, S.shifted_taps(x, blk['shifts']), dZ, dx, blk,
                               S.bias_of(var, l), None, np.float64)
        ref = S.device_sections(g, l, K, l == L - 1)
        assert sorted(ref) == sorted(k for k in out if k not in ('da_f', 'da_g', 'dx'))
        for k in ref:
            same(out[k], ref[k], (l, k))
        dx = out['dx']
    # dx_0 pins the chain of dx through every layer: the causal layer's gradient
    enc = c['net_in']
    for kk, sh in enumerate(S.tap_shifts(K, 1)):
        want = g['causal_layer']['filter'][kk]
        got = S.shift(enc, sh).reshape(B * T, -1).T @ dx.reshape(B * T, -1)
        same(got, want, ('causal', kk))


def test_float32_restatement_is_float32_and_close():
    """The float32 evaluation the GPU bounds are measured with really runs in
    float32 (asserted inside layer_forward / layer_backward) and differs from
    float64 by rounding, not by a formula."""
    cfg = S.CASES['mid'][0]
    var = S.saturated_variables(cfg, 6.0)
    codes, _, _ = S.case_inputs('mid')
    c64 = S.forward_chain(cfg, var, codes, None, np.float64)
    x = c64['layers'][5]['x'].astype(np.float32)
    blk = S.block_of(var, 5, cfg['dilations'], 2)
    xs = S.shifted_taps(x, blk['shifts'])
    a = S.layer_forward(x, xs, blk, S.bias_of(var, 5), None, np.float32)
    b = S.layer_forward(x, xs, blk, S.bias_of(var, 5), None, np.float64)
    for u, v in zip(a, b):
        assert u.dtype == np.float32 and v.dtype == np.float64
        assert 0 < np.abs(u - v).max() < 1e-4


def test_xent_restatement_matches_the_oracle_loss():
    """sat_ref.xent (float64) on the oracle's logits: its loss and dlogits."""
    cfg = S.CASES['tiny'][0]
    var = S.saturated_variables(cfg, 3.0)
    codes, audio, _ = S.case_inputs('tiny')
    B, T = codes.shape
    for quirk in (True, False):
        loss, g, c = O.loss_and_grads(cfg, var, audio, dtype=np.float64,
                                      tf_xent_zero_label_quirk=quirk,
                                      return_cache=True)
        tot, dl, _ = S.xent(c['logits'], codes, None, 1.0 / (B * T), quirk,
                            np.float64)
        assert abs(tot / (B * T) - loss) < 1e-12
        want = c['h2'].reshape(B * T, -1).T @ dl.reshape(B * T, -1)
        assert np.abs(want - g['postprocessing']['postprocess2'][0]).max() < 1e-12
