"""Inputs shared by the mixture-of-logistics tests (host and GPU): synthetic
head outputs that reach every branch of the row loss, the sampling fixtures
whose draws the host test shows to lie off every rounding boundary, and the
error yardstick of the kernel tests."""
import numpy as np

import mol_ref as R

LSM = -14.0
EDGE_LEVELS = (0, 1, 65534, 65535)


def padded(K):
    return (K + 3) // 4 * 4


def kernel_case(B, T, K, ld_gap=0, seed=0, lsm=LSM):
    """(logits float32 [B * T, 3 Kp + ld_gap], levels int32 [B, T]).  Targets
    cycle through levels 0, 1, 65534, 65535 and interior ones; beta_raw sits
    at, below (down to -80) and above the clamp; mu sits on the target, a few
    bins off and far off, so that |c - mu| e^-beta reaches 1e6; the gap
    columns hold NaN."""
    rng = np.random.default_rng([seed, B, T, K])
    N, Kp = B * T, padded(K)
    lv = rng.integers(2, 65534, (B, T))
    flat = lv.reshape(-1)
    for i, e in enumerate(EDGE_LEVELS):
        flat[i + 1::7][:max(1, N // 9)] = e       # (row t is scored on t + 1)
    c = R.centres(flat)
    tgt = np.concatenate([c[1:], c[:1]])[:, None]
    lg = np.full((N, 3 * Kp + ld_gap), np.nan, np.float32)
    lg[:, :3 * Kp] = 0
    lg[:, :K] = rng.normal(0, 2, (N, K))
    beta = rng.uniform(-16, 1, (N, K))
    kind = rng.integers(0, 8, (N, K))
    beta[kind == 0] = lsm                        # at the clamp
    beta[kind == 1] = rng.uniform(-80, lsm - 1e-3, (kind == 1).sum())
    beta[kind == 2] = rng.uniform(lsm, lsm + 2, (kind == 2).sum())
    scale = np.exp(np.maximum(beta, lsm))
    off = rng.normal(0, 1, (N, K)) * scale * rng.choice(
        [0.0, 0.5, 3.0, 30.0], (N, K))
    far = rng.integers(0, 6, (N, K)) == 0
    mu = np.where(far, rng.uniform(-1.2, 1.2, (N, K)), tgt + off)
    lg[:, Kp:Kp + K] = mu
    lg[:, 2 * Kp:2 * Kp + K] = beta
    # padded columns: poison that must be neither read nor kept
    for blk in range(3):
        lg[:, blk * Kp + K:(blk + 1) * Kp] = np.nan
    return lg, lv.astype(np.int32)


def scales(logits, target, K, lsm, inv):
    """The magnitude of the terms each output of a row is a sum of (float64):
    dict nll [N], pi [N], mu [N], beta [N].  A float32 evaluation of a sum
    cannot be closer than one ulp of its largest term: nll = -(mw + log sw)
    with w_k = log_softmax(pi)_k + lp_k, of which only components that carry
    posterior weight matter; g_pi = (p - r) inv with p, r <= 1; g_mu = r is
    (sb - sna) inv with sigmoids <= 1; g_beta = r (b sb - a sna - gt) inv."""
    Kp = padded(K)
    lg = np.asarray(logits, np.float64)
    pi, mu = lg[:, :K], lg[:, Kp:Kp + K]
    beta = np.maximum(lg[:, 2 * Kp:2 * Kp + K], lsm)
    t = np.where(target >= 0, target, 1)
    c = R.centres(t)[:, None]
    is_ = np.exp(-beta)
    a, b = (c + R.H - mu) * is_, (c - R.H - mu) * is_
    import torch
    with torch.no_grad():
        lp = R.log_bin(torch.as_tensor(t).reshape(-1, 1),
                       torch.as_tensor(mu), torch.as_tensor(beta)).numpy()
    lsp = pi - pi.max(1, keepdims=True)
    lsp = lsp - np.log(np.exp(lsp).sum(1, keepdims=True))
    w = lsp + lp
    r = np.exp(w - w.max(1, keepdims=True))
    r /= r.sum(1, keepdims=True)
    live = r > 2.0 ** -24
    big = np.maximum(np.abs(a), np.abs(b))
    return dict(
        nll=np.maximum(1.0, np.where(live, np.maximum(np.abs(lp), np.abs(lsp)),
                                     0).max(1)),
        pi=np.full(len(lg), abs(inv)),
        mu=(r * is_).max(1) * abs(inv),
        beta=(r * np.maximum(big, 1.0)).max(1) * abs(inv))


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)
                      ).astype(np.float64)


def worst_ratio(got, ref32, ref64, scale_rows):
    """The yardstick: every entry of `got` [N, k] must lie within FOUR TIMES
    the larger of (the float32 numpy restatement's own largest error against
    float64 in that row) and (one float32 ulp of the row's scale).  Returns
    the largest error seen as a fraction of that bound."""
    got, ref32, ref64 = (np.asarray(x, np.float64).reshape(len(scale_rows), -1)
                         for x in (got, ref32, ref64))
    own = np.abs(ref32 - ref64).max(1)
    bound = 4.0 * np.maximum(own, ulp32(scale_rows))
    err = np.abs(got - ref64).max(1)
    assert np.isfinite(got).all()
    return float((err / bound).max())


# ---- sampling fixtures: [R, 3, K] float32 parameters as wn_mol_params_row
# writes them, one (seed, counter) per row
def sample_fixture(K, R=96, seed=5):
    rng = np.random.default_rng([seed, K])
    p = np.empty((R, 3, K), np.float32)
    pi = rng.normal(0, 2, (R, K))
    pi -= np.log(np.exp(pi).sum(1, keepdims=True))
    p[:, 0] = pi
    p[:, 1] = rng.uniform(-1.1, 1.1, (R, K))
    p[:, 2] = rng.uniform(-14, -2, (R, K))
    if K > 1:
        p[::5, 0, 1:] = -np.inf            # a component of weight exactly 0
        p[::5, 0, 0] = 0
    seeds = rng.integers(0, 2 ** 63, R, dtype=np.int64)
    seeds[1::7] = -seeds[1::7]             # (bit patterns above 2^63 too)
    counters = rng.integers(0, 2 ** 40, R, dtype=np.int64)
    counters[:4] = (0, 1, 2 ** 31, 2 ** 40)
    return p, seeds, counters


SAMPLE_K = (1, 4, 10, 32)
SAMPLE_TEMPERATURES = (1.0, 0.7, 0.0)
