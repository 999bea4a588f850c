"""Saturated inputs and plain restatements for the gate non-linearities (test
infrastructure only; numpy, the oracle through tests/util).

The parity tests elsewhere build Xavier weights and N(0, 0.1) biases: tanh and
sigmoid stay in their near-linear region (max |tanh| 0.98, sigmoid within
[0.1, 0.93]).  `saturated_variables` scales the gate weights by a gain and
plants exact extremes in single channels, so that a trained network's regime --
tanh at +-1, sigmoid at 0 and 1, a float32 sigmoid of exactly 0 -- is reached.

`layer_forward` / `layer_backward` restate ONE residual block in float64 or
float32 from GIVEN inputs.  The GPU tests feed them the device's own planes of
every layer, so nothing is chained: errors do not compound over depth and the
comparison stays well conditioned at any gain.  tanh and sigmoid are always
recomputed from x_l (np.tanh, 1 / (1 + exp(-a))), never recovered as z / sigmoid
as the device does.  tests/test_saturation_host.py pins both to the oracle's
per-layer cache and asserts that every case below reaches the regime.
"""
import numpy as np

from util import O, TINY, MID, cfg_with

# (layer, bias, channel, value): see the module docstring of
# tests/test_saturation_host.py for what each forces.  Channels < 8: below the
# smallest dilation_channels of any case.
PLANTS = [(1, 'gate_bias', 0, -120.0),     # float32 sigmoid exactly 0
          (1, 'gate_bias', 1, 120.0),      # sigmoid exactly 1
          (2, 'filter_bias', 2, -60.0),    # tanh -1
          (2, 'filter_bias', 3, 60.0),     # tanh +1
          (3, 'gate_bias', 4, -60.0)]      # sigmoid ~ 1e-26: inside (1e-30, 1e-22)
NOBIAS_GAIN = 6.0


def _xavier(rng, shape):
    lim = np.sqrt(6.0 / (shape[-2] + shape[-1]))
    return rng.uniform(-lim, lim, size=shape)


def saturated_variables(cfg, gain, seed=0):
    """The oracle's variables (float64, biases N(0, 0.1)) with every layer's
    filter / gate tensor -- and the GC / LC filter and gate weights -- times
    `gain`, and PLANTS written into the biases.  A model without biases gets no
    plants and gain 6.  cfg['local_condition_channels'] adds lc_filtweights /
    lc_gateweights [Lc, D] per layer (the oracle has none)."""
    ub = bool(cfg.get('use_biases', False))
    if not ub:
        gain = NOBIAS_GAIN
    var = O.create_variables(cfg, seed=seed, dtype=np.float64,
                             bias_scale=0.1 if ub else 0.0)
    Lc = cfg.get('local_condition_channels')
    rng = np.random.default_rng(seed + 1000)
    for cur in var['dilated_stack']:
        for k in ('filter', 'gate', 'gc_filtweights', 'gc_gateweights'):
            if k in cur:
                cur[k] = cur[k] * gain
        if Lc:
            D = cfg['dilation_channels']
            cur['lc_filtweights'] = _xavier(rng, (Lc, D)) * gain
            cur['lc_gateweights'] = _xavier(rng, (Lc, D)) * gain
    if ub:
        for l, name, ch, val in PLANTS:
            var['dilated_stack'][l][name][ch] = val
    return var


# --------------------------------------------------------------- one block
def tap_shifts(K, d):
    """Rows tap k of a K-tap causal convolution of dilation d looks back
    (oracle.causal_conv: TF's SAME centring delays K > 2 by (K - 1) // 2)."""
    return [(K - 1 - k + (K - 1) // 2) * d for k in range(K)]


def shift(x, s):
    """x[t - s] with zeros before the clip start; x [B, T, C]."""
    out = np.zeros_like(x)
    T = x.shape[1]
    if s < T:
        out[:, s:] = x[:, :T - s]
    return out


def unshift(y, s):
    """y[t + s] with zeros past the clip end (the transpose of `shift`)."""
    out = np.zeros_like(y)
    T = y.shape[1]
    if s < T:
        out[:, :T - s] = y[:, s:]
    return out


def shifted_taps(x, shifts):
    return [shift(x, s) for s in shifts]


def block_of(var, l, dilations, K):
    """Layer l's weights as layer_forward / layer_backward take them."""
    cur = var['dilated_stack'][l]
    last = l == len(dilations) - 1
    return dict(filter=cur['filter'], gate=cur['gate'],
                dense=None if last else cur['dense'][0],
                dense_bias=None if last else cur.get('dense_bias'),
                shifts=tap_shifts(K, int(dilations[l])))


def bias_of(var, l):
    cur = var['dilated_stack'][l]
    if 'filter_bias' not in cur:
        return None
    return cur['filter_bias'], cur['gate_bias']


def lc_addend(var, l, lc):
    """The LC rows' filter | gate addends of layer l; lc [B, T, Lc]."""
    cur = var['dilated_stack'][l]
    lc = np.asarray(lc, np.float64)
    return lc @ cur['lc_filtweights'], lc @ cur['lc_gateweights']


def _c(a, dtype):
    return None if a is None else np.asarray(a).astype(dtype)


def layer_forward(x_l, x_l_shifted, block, bias_fg, lc_add, dtype):
    """(tanh, sigmoid, z, x_{l+1}) of ONE residual block, evaluated in `dtype`
    (float64 or float32) from its input x_l [B, T, R] and the input as every
    tap sees it, x_l_shifted[k] = shift(x_l, block['shifts'][k]).  bias_fg:
    (filter, gate) biases broadcastable to [B, T, D] or None; lc_add: (filter,
    gate) addends [B, T, D] or None.  x_{l+1} is None for the last layer."""
    xs = [_c(v, dtype) for v in x_l_shifted]
    Wf, Wg = _c(block['filter'], dtype), _c(block['gate'], dtype)
    a_f = sum(xs[k] @ Wf[k] for k in range(len(xs)))
    a_g = sum(xs[k] @ Wg[k] for k in range(len(xs)))
    for add in (bias_fg, lc_add):
        if add is not None:
            a_f = a_f + _c(add[0], dtype)
            a_g = a_g + _c(add[1], dtype)
    one = dtype(1)
    with np.errstate(over='ignore'):        # exp(+large) = inf: sigmoid 0
        t, s = np.tanh(a_f), one / (one + np.exp(-a_g))
    z = t * s
    xn = None
    if block['dense'] is not None:
        xn = _c(x_l, dtype) + z @ _c(block['dense'], dtype)
        if block['dense_bias'] is not None:
            xn = xn + _c(block['dense_bias'], dtype)
    assert all(a.dtype == dtype for a in (t, s, z))
    return t, s, z, xn


def layer_backward(x_l, x_l_shifted, dZ_l, dx_next, block, bias_fg, lc_add,
                   dtype):
    """The gradients of ONE residual block in `dtype` from x_l, dZ_l (the skip
    path's gradient into z_l) and dx_{l+1} (None for the last layer):
    da_f = dz s (1 - t^2), da_g = dz t s (1 - s) with dz = dZ_l + dx_{l+1} Wd^T
    and t, s recomputed from x_l.  Returns a dict: da_f, da_g [B, T, D]; Wf<k>,
    Wg<k> [R, D] per tap; bf, bg [D]; with dx_{l+1} also Wd [D, R], bd [R];
    dx_l [B, T, R]."""
    t, s, z, _ = layer_forward(x_l, x_l_shifted, block, bias_fg, lc_add, dtype)
    xs = [_c(v, dtype) for v in x_l_shifted]
    Wf, Wg = _c(block['filter'], dtype), _c(block['gate'], dtype)
    dz = _c(dZ_l, dtype)
    dxn = _c(dx_next, dtype)
    if dxn is not None:
        dz = dz + dxn @ _c(block['dense'], dtype).T
    one = dtype(1)
    da_f = dz * s * (one - t * t)
    da_g = dz * t * s * (one - s)
    f2 = lambda a: a.reshape(-1, a.shape[-1])
    out = dict(da_f=da_f, da_g=da_g, bf=f2(da_f).sum(0), bg=f2(da_g).sum(0))
    dx = np.zeros(xs[0].shape, dtype) if dxn is None else dxn.copy()
    for k, sh in enumerate(block['shifts']):
        out['Wf%d' % k] = f2(xs[k]).T @ f2(da_f)
        out['Wg%d' % k] = f2(xs[k]).T @ f2(da_g)
        dx += unshift(da_f @ Wf[k].T + da_g @ Wg[k].T, sh)
    if dxn is not None:
        out['Wd'] = f2(z).T @ f2(dxn)
        out['bd'] = f2(dxn).sum(0)
    out['dx'] = dx
    assert all(v.dtype == dtype for v in out.values())
    return out


def device_sections(gtree, l, K, last):
    """The same names from a gradient tree shaped like the model's
    `variables` (numpy): what layer_backward's weight gradients compare to."""
    cur = gtree['dilated_stack'][l]
    out = {}
    for k in range(K):
        out['Wf%d' % k] = cur['filter'][k]
        out['Wg%d' % k] = cur['gate'][k]
    if 'filter_bias' in cur:
        out['bf'], out['bg'] = cur['filter_bias'], cur['gate_bias']
    if not last:
        out['Wd'] = cur['dense'][0]
        if 'dense_bias' in cur:
            out['bd'] = cur['dense_bias']
    return out


# ------------------------------------------------------ the chained network
def forward_chain(cfg, var, codes, lc=None, dtype=np.float64):
    """The whole network by chaining layer_forward over one-hot `codes`
    [B, T] (LC rows lc [B, T, Lc] for an LC model; no global conditioning):
    {'layers': [{x, tanh, sig, z}], 'total', 'logits'} like the cache of
    oracle.network_forward(keep=True)."""
    var = O.cast_variables(var, dtype)
    Q, K, dil = cfg['quantization_channels'], cfg['filter_width'], cfg['dilations']
    x = O.causal_conv(O.one_hot(np.asarray(codes), Q, dtype),
                      var['causal_layer']['filter'], 1)
    layers, total = [], None
    for l in range(len(dil)):
        blk = block_of(var, l, dil, K)
        add = None if lc is None else tuple(
            a.astype(dtype) for a in lc_addend(var, l, lc))
        t, s, z, xn = layer_forward(x, shifted_taps(x, blk['shifts']), blk,
                                    bias_of(var, l), add, dtype)
        layers.append(dict(x=x, tanh=t, sig=s, z=z))
        cur = var['dilated_stack'][l]
        skip = z @ cur['skip'][0]
        if 'skip_bias' in cur:
            skip = skip + cur['skip_bias']
        total = skip if total is None else total + skip
        x = xn
    p = var['postprocessing']
    ub = 'postprocess1_bias' in p
    c1 = np.maximum(total, 0) @ p['postprocess1'][0]
    if ub:
        c1 = c1 + p['postprocess1_bias']
    logits = np.maximum(c1, 0) @ p['postprocess2'][0]
    if ub:
        logits = logits + p['postprocess2_bias']
    return dict(layers=layers, total=total, logits=logits)


def softmax64(logits):
    """The generator's probabilities: float64 softmax cast to float32."""
    return O._softmax64(logits)


# -------------------------------------------------------------- the regime
def coverage(layers):
    """Where the gate activations of a float64 forward cache sit."""
    t = np.concatenate([c['tanh'].reshape(-1) for c in layers])
    s = np.concatenate([c['sig'].reshape(-1) for c in layers])
    return dict(
        tanh_sat=float((np.abs(t) > 0.99).mean()),
        tanh_lin=float((np.abs(t) < 0.5).mean()),
        sig_lo=float((s < 1e-3).mean()), sig_hi=float((s > 0.999).mean()),
        sig_zero32=int((s < 1e-45).sum()),
        sig_guard=int(((s > 1e-30) & (s < 1e-22)).sum()),
        sig_mid=float(((s > 0.1) & (s < 0.9)).mean()))


def assert_coverage(cov, what=''):
    """The conditions every saturated case must meet (asserted on the CPU for
    every case the GPU tests run)."""
    assert cov['tanh_sat'] >= 0.25, (what, cov)
    assert cov['tanh_lin'] >= 0.05, (what, cov)     # the linear region stays covered
    assert cov['sig_lo'] >= 0.02 and cov['sig_hi'] >= 0.02, (what, cov)
    assert cov['sig_zero32'] >= 1, (what, cov)      # exactly 0 in float32
    assert cov['sig_guard'] >= 1, (what, cov)       # where + 1e-30 changes z / s
    assert cov['sig_mid'] >= 0.25, (what, cov)


# ------------------------------------------------- the cases of the GPU tests
# name -> (cfg, T, gains, kind).  kind 'train': audio uniform(-1, 1) [B, T];
# 'gen': B = 1, a code trace of sum(dilations) + 2 + 25 (T is ignored).
# Gains 3 and 6, except where a case cannot meet assert_coverage with them
# (measured on the float64 oracle): T = 20 and three taps reach 25 % saturated
# tanh only from gain 4 (most taps see the zero padding / the receptive field
# is wider), the LC addend pushes gain 6 below 25 % mid-range sigmoids.
_R64 = dict(residual_channels=64, dilation_channels=64)
CASES = {
    'mid': (cfg_with(MID, batch_size=2), 150, (3.0, 6.0), 'train'),
    'mid_T20': (cfg_with(MID, batch_size=2), 20, (4.0, 6.0), 'train'),
    'mid_S512': (cfg_with(MID, batch_size=2, skip_channels=512), 150,
                 (3.0, 6.0), 'train'),
    'mid_k3': (cfg_with(MID, batch_size=2, filter_width=3), 150, (4.0, 6.0),
               'train'),
    'r64': (cfg_with(MID, batch_size=2, skip_channels=32, **_R64), 150,
            (3.0, 6.0), 'train'),
    'mid_lc': (cfg_with(MID, batch_size=2, local_condition_channels=16), 150,
               (2.0, 3.0), 'train'),
    'tiny': (cfg_with(TINY, batch_size=2), 37, (3.0,), 'train'),
    'gen_mid': (cfg_with(MID, batch_size=1), None, (3.0, 6.0), 'gen'),
    'gen_r64': (cfg_with(MID, batch_size=1, skip_channels=128, **_R64), None,
                (3.0,), 'gen'),
    'gen_lc': (cfg_with(MID, batch_size=1, local_condition_channels=16), None,
               (3.0,), 'gen'),
}
# LC rows are N(0, 1) times this: with 16 channels the addend alone has a
# standard deviation of 1.1 x gain, enough to saturate gates by itself
LC_ROW_SCALE = 1.5


def case_inputs(name, stream=0):
    """(codes int32 [B, T], audio float32 [B, T] or None, lc float32
    [B, T, Lc] or None) of a case; `stream`: another draw (batched
    generation)."""
    cfg, T, _, kind = CASES[name]
    B, Q = cfg['batch_size'], cfg['quantization_channels']
    if kind == 'train':
        audio = np.random.default_rng(7 + stream).uniform(
            -1, 1, (B, T)).astype(np.float32)
        codes = O.mu_law_encode(audio, Q)
    else:
        T = sum(cfg['dilations']) + 2 + 25
        audio = None
        codes = np.random.default_rng(9 + stream).integers(
            0, Q, (B, T)).astype(np.int32)
    lc = None
    Lc = cfg.get('local_condition_channels')
    if Lc:
        lc = (LC_ROW_SCALE * np.random.default_rng(11 + stream).standard_normal(
            (B, T, Lc))).astype(np.float32)
    return codes, audio, lc


# ------------------------------------------------- softmax cross-entropy
def xent(logits, codes, lengths, inv_n, quirk, dtype):
    """Loss sum and dlogits [B, T, Q] of the training step's softmax
    cross-entropy in `dtype`: row (b, t) has the target codes[b, t + 1] while
    t + 1 < lengths[b] (lengths None: T), the row after has none (with `quirk`
    it still back-propagates its softmax), rows past it are padding (zeros).
    inv_n: the float32 factor the device scales dlogits by.  Returns (sum of
    the rows' losses, dlogits, the rows' losses [B, T])."""
    x = np.asarray(logits).astype(dtype)
    B, T, Q = x.shape
    codes = np.asarray(codes)
    ln = np.full(B, T) if lengths is None else np.clip(np.asarray(lengths), 0, T)
    t = np.arange(T)[None, :]
    live = t < ln[:, None]
    label = np.full((B, T), -1, np.int64)
    label[:, :-1] = codes[:, 1:]
    label[t + 1 >= ln[:, None]] = -1
    has = (label >= 0) & (label < Q)
    m = x.max(-1, keepdims=True)
    e = np.exp(x - m)
    se = e.sum(-1, keepdims=True, dtype=dtype)
    lse = (m + np.log(se))[..., 0]
    ll = np.take_along_axis(x, np.where(has, label, 0)[..., None], -1)[..., 0]
    rows = np.where(has, lse - ll, dtype(0)).astype(dtype)
    back = (has | bool(quirk)) & live
    p = np.where(back[..., None], e / se, dtype(0)).astype(dtype)
    b_i, t_i = np.nonzero(has)
    p[b_i, t_i, label[b_i, t_i]] -= dtype(1)
    g = (p * dtype(inv_n)).astype(dtype)
    return rows.sum(dtype=dtype), g, rows
