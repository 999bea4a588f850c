"""The host restatement of fast generation's draw (tests/draw_ref.py) against
published SplitMix64 values and a direct float64 evaluation of the
reference's temperature rule (generate.py:228-240).  The GPU tests compare
every drawn code with it, so it has to be right on its own."""
import numpy as np
import pytest

import draw_ref as D

TAUS = (1.0, 0.7, 0.05, 3.0, 100.0)


def _softmax32(logits):
    l = np.asarray(logits, np.float64)
    e = np.exp(l - l.max())
    return (e / e.sum()).astype(np.float32)


def _cliff(Q, rng):
    """One code at +120, a few at +110, the rest at 0: float32 probabilities
    exactly 0 at both ends and in the middle."""
    l = np.zeros(Q)
    l[rng.integers(1, Q - 1)] = 120.0
    l[rng.choice(np.arange(1, Q - 1), 3, replace=False)] = 110.0
    return l


def _reference_weights(p32, T):
    # generate.py:229-233 in float64: log(p) / T, minus logaddexp.reduce, exp
    with np.errstate(divide='ignore'):
        s = np.log(np.asarray(p32, np.float64)) / T
    s = s - np.logaddexp.reduce(s)
    return np.exp(s)


def test_splitmix64_published_values():
    # the SplitMix64 stream from state 0: first and second outputs
    assert D.splitmix64(0) == 0xe220a8397b1dcdaf
    assert D.splitmix64(0x9E3779B97F4A7C15) == 0x6e789e6aa1b965f4
    # ... and the first five outputs from state 1234567
    s, out = 1234567, []
    for _ in range(5):
        out.append(D.splitmix64(s))
        s = (s + 0x9E3779B97F4A7C15) % 2 ** 64
    assert out == [6457827717110365317, 3203168211198807973,
                   9817491932198370423, 4593380528125082431,
                   16408922859458223821]
    # the array form gives the same values as the scalar one
    x = [0, 1, 2 ** 63, 2 ** 64 - 1, 1234567]
    assert [int(v) for v in D.splitmix64(np.array(x, np.uint64))] == \
        [D.splitmix64(v) for v in x]


def test_uniform_is_53_bits_of_the_counter_hash():
    for seed in (0, 2, 11, 2 ** 64 - 1):
        for c in (0, 1, 15999, 2 ** 31 - 1):
            r = D.splitmix64(seed ^ D.splitmix64(c))
            assert D.uniform(seed, c) == (r >> 11) * 2.0 ** -53
    u = D.uniform(5, np.arange(100))
    assert u.dtype == np.float64 and u.shape == (100,)
    assert u[37] == D.uniform(5, 37)


@pytest.mark.parametrize('tau', TAUS)
def test_weights_match_generate_py_rule(tau):
    rng = np.random.default_rng(int(tau * 1000))
    for Q in (100, 256, 1024):
        for kind in ('random', 'cliff'):
            logits = rng.normal(0, 4, Q) if kind == 'random' else _cliff(Q, rng)
            p = _softmax32(logits)
            if kind == 'cliff':
                assert (p == 0).sum() >= Q - 4 and p[0] == 0 and p[-1] == 0
            w = D.weights(p, tau)
            if tau == 1.0:
                assert np.array_equal(w, p.astype(np.float64))
            ref = _reference_weights(p, tau)
            got = w / w.sum()
            assert np.array_equal(got == 0, ref == 0), (Q, kind)
            assert np.array_equal(w[p == 0], np.zeros(int((p == 0).sum())))
            nz = ref > 0
            rel = np.abs(got[nz] - ref[nz]) / ref[nz]
            assert rel.max() < 1e-12, (Q, kind, float(rel.max()))
    # rows are independent: a batch of distributions equals one at a time
    P = np.stack([_softmax32(rng.normal(0, 4, 64)) for _ in range(5)])
    W = D.weights(P, tau)
    for i in range(5):
        assert np.array_equal(W[i], D.weights(P[i], tau))


def test_pick_never_takes_a_zero_weight_code():
    rng = np.random.default_rng(3)
    below_one = 1.0 - 2.0 ** -53
    for Q in (2, 7, 100, 256):
        for _ in range(50):
            w = rng.uniform(0, 1, Q) * (rng.uniform(size=Q) < 0.3)
            w[0] = w[-1] = 0.0                      # zero weight at both ends
            if Q > 2:
                w[Q // 2] = 0.0                      # ... and in the middle
                w[rng.integers(1, Q - 1)] = rng.uniform(0.1, 1)
            else:
                w[rng.integers(0, 2)] = 1.0
            nz = np.nonzero(w > 0)[0]
            for u in (0.0, below_one, *rng.uniform(size=20)):
                k = int(D.pick(w, u))
                assert w[k] > 0, (Q, u, k)
            assert D.pick(w, 0.0) == nz[0]
            assert D.pick(w, below_one) == nz[-1]
    # the inverse CDF itself: [0.2, 0, 0.3, 0.5]
    w = np.array([0.2, 0.0, 0.3, 0.5])
    for u, k in ((0.0, 0), (0.1999, 0), (0.2, 2), (0.49, 2), (0.5, 3),
                 (below_one, 3)):
        assert D.pick(w, u) == k, (u, k)
    assert abs(float(D.margin(w, 0.45)) - 0.05) < 1e-15
    assert D.boundary_codes(w, 0.21) == (0, 2)
    # batch form: one row per draw
    W = np.stack([w, w[::-1]])
    assert list(D.pick(W, np.array([0.1, 0.1]))) == [0, 0]
    assert list(D.pick(W, np.array([0.25, 0.85]))) == [2, 3]


def test_restated_uniforms_chi_square():
    # 16000 uniforms (a 16000-sample run's counters) in 64 bins: chi-square
    # below the 0.999 quantile of 63 degrees of freedom (103.4)
    for seed in (2, 11, 123):
        u = D.uniform(seed, np.arange(16000))
        assert u.min() >= 0.0 and u.max() < 1.0
        n = np.bincount((u * 64).astype(np.int64), minlength=64)
        chi2 = float(((n - 250.0) ** 2 / 250.0).sum())
        assert chi2 < 103.4, (seed, chi2)


def test_check_draws_catches_a_shifted_counter_and_a_wrong_temperature_rule():
    """The comparison the GPU tests make, on draws made here: it accepts the
    restated codes and rejects the draw of the neighbouring counter, the
    temperature applied as p ** tau, and a draw of a probability-0 code."""
    rng = np.random.default_rng(7)
    N, Q, seed = 2000, 256, 4
    P = np.stack([_softmax32(rng.normal(0, 4, Q)) for _ in range(N)])
    ctr = np.arange(1, N + 1)
    for tau in (1.0, 0.7, 3.0):
        good = D.pick(D.weights(P, tau), D.uniform(seed, ctr))
        assert D.check_draws(good, P, tau, seed, ctr) == 0
        shifted = D.pick(D.weights(P, tau), D.uniform(seed, ctr + 1))
        with pytest.raises(AssertionError, match='restated code'):
            D.check_draws(shifted, P, tau, seed, ctr)
        if tau != 1.0:
            pw = P.astype(np.float64) ** tau
            wrong = D.pick(pw, D.uniform(seed, ctr))
            with pytest.raises(AssertionError, match='restated code'):
                D.check_draws(wrong, P, tau, seed, ctr)
    cliff = np.stack([_softmax32(_cliff(Q, rng)) for _ in range(N)])
    codes = D.pick(D.weights(cliff, 100.0), D.uniform(seed, ctr))
    assert D.check_draws(codes, cliff, 100.0, seed, ctr) == 0
    codes[5] = 0                                       # p == 0 there
    with pytest.raises(AssertionError, match='probability 0'):
        D.check_draws(codes, cliff, 100.0, seed, ctr)
