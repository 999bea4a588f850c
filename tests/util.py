"""Shared test helpers: build the HIP model and the CPU oracle on identical
weights.  (tests/ may import oracle/; the product never does.)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'tensorflow-wavenet_amd')
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import wavenet_oracle as O  # noqa: E402

TINY = dict(dilations=[1, 2, 4, 8, 1, 2, 4, 8], filter_width=2,
            residual_channels=8, dilation_channels=8, skip_channels=16,
            quantization_channels=16, use_biases=True)
MID = dict(dilations=[1, 2, 4, 8, 16, 32, 64, 1, 2, 4, 8, 16, 32, 64],
           filter_width=2, residual_channels=32, dilation_channels=32,
           skip_channels=64, quantization_channels=256, use_biases=True)
DEFAULT = dict(dilations=[2 ** i for i in range(10)] * 5, filter_width=2,
               residual_channels=32, dilation_channels=32, skip_channels=512,
               quantization_channels=256, use_biases=True)

# Dilation lists that are not powers of two (tests/test_dilations_host.py
# counts, per list and clip length, the tile-layer pairs of the persistent
# stack launches whose dilated tap straddles two foreign tiles, or starts
# inside a later tile):
#   DIL_A  96 is tile-aligned without being a power of two; 31, 33 and 63 sit
#          one row off a tile edge            (T = 333 / 301; T = 47: d >= T)
#   DIL_B  the 16-row geometry                (T = 150)
#   DIL_C  taps far behind, 513 one off a power of two; receptive field 2605
#          (T = 1100)
#   DIL_GEN  the generators' rings: no cursor wraps in phase with another
DIL_A = [33, 48, 1, 100, 7, 63, 96, 3, 40, 31]
DIL_B = [17, 24, 5, 40, 15, 50, 9]
DIL_C = [33, 1000, 48, 1, 100, 7, 63, 96, 3, 700, 513, 40]
DIL_GEN = [3, 5, 33, 7, 48, 17]


def cfg_with(base, **kw):
    c = dict(base)
    c.update(kw)
    return c


def synth_audio(B, T, seed=1234, sample_rate=16000):
    """BASELINE.md synthetic clips: sine + noise, clipped to [-1, 1]."""
    rng = np.random.default_rng(seed)
    t = np.arange(T)
    out = np.empty((B, T), np.float32)
    for b in range(B):
        f = 110.0 * 2 ** (b / 12.0)
        x = 0.5 * np.sin(2 * np.pi * f * t / sample_rate) + \
            0.05 * rng.standard_normal(T)
        out[b] = np.clip(x, -1, 1)
    return out


def model_kwargs(cfg):
    keys = ['batch_size', 'dilations', 'filter_width', 'residual_channels',
            'dilation_channels', 'skip_channels', 'quantization_channels',
            'use_biases', 'scalar_input', 'initial_filter_width',
            'global_condition_channels', 'global_condition_cardinality',
            'residual_postproc', 'output_mixture', 'mixture_log_scale_min']
    return {k: cfg[k] for k in keys if k in cfg}


def build_pair(cfg, seed=0, bias_scale=0.1):
    """(HIP model, oracle variables float64) with identical weights."""
    from wavenet import WaveNetModel
    var = O.create_variables(cfg, seed=seed, dtype=np.float64,
                             bias_scale=bias_scale if cfg.get('use_biases')
                             else 0.0)
    net = WaveNetModel(**model_kwargs(cfg))
    net.load_nested(var)
    return net, var


def flat_named(tree):
    return O.flatten_variables(tree)


def tree_to_numpy(tree):
    if isinstance(tree, dict):
        return {k: tree_to_numpy(v) for k, v in tree.items()}
    if isinstance(tree, list):
        return [tree_to_numpy(v) for v in tree]
    return tree.detach().cpu().numpy().astype(np.float64)


def oracle_grads_at_device_kinks(net, cfg, var, audio, ids=None, l2=None,
                                 kink_tol=2e-5, cache=None, **kw):
    """float64 oracle loss / gradients evaluated with the DEVICE's ReLU
    decisions (see oracle.loss_and_grads: relu_masks).  First checks that the
    device's masks differ from the oracle's own only where the oracle's
    pre-activation is within `kink_tol` of zero (forward rounding), i.e. that
    passing them changes which subgradient is taken at a kink and nothing
    else.  `cache`: the float64 forward cache of O.loss(keep=True) on the same
    inputs when the caller already holds it.  Returns (loss, grads, cache,
    n_flipped)."""
    B = cfg['batch_size']
    c = cache
    if c is None:
        _, c = O.loss(cfg, var, audio, ids, l2, np.float64, keep=True)
    T = c['logits'].shape[1]
    ws = [w for w in net._ws.values() if w.T == T and w.training][0]
    S = cfg['skip_channels']
    m_total = (ws.h1 > 0).cpu().numpy().reshape(B, T, S)
    src = ws.c1 if cfg.get('residual_postproc', False) else ws.h2
    m_c1 = (src > 0).cpu().numpy().reshape(B, T, S)
    flips = 0
    for m, ref in ((m_total, c['total']), (m_c1, c['c1'])):
        diff = m != (ref > 0)
        flips += int(diff.sum())
        assert np.abs(ref[diff]).max(initial=0.0) < kink_tol, \
            float(np.abs(ref[diff]).max())
    loss, g = O.loss_and_grads(cfg, var, audio, ids, l2=l2, dtype=np.float64,
                               relu_masks=dict(total=m_total, c1=m_c1), **kw)
    return loss, g, c, flips
