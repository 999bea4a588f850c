"""wavenet/resample.py without a device: limits, the tap design against
scipy's firwin, tests/resample_ref.py against scipy's resample_poly, the numpy
float32 rule against the float64 restatement, and the binding table against
include/wavenet_resample.h."""
import glob
import os
import re

import numpy as np
import pytest

import resample_ref as R
from util import ROOT

HEADER = 'wavenet_resample.h'
RATIOS = [(5, 8), (5, 12), (5, 4), (100, 441), (1, 1)]


def _rates(up, down):
    return down * 100, up * 100


def _signal(n, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return (0.5 * np.sin(0.05 * t) + 0.2 * rng.standard_normal(n)
            ).astype(np.float32)


# ------------------------------------------------------------------ limits
def test_limits_come_before_the_library(monkeypatch):
    from wavenet import _lib, resample
    monkeypatch.setattr(_lib, 'load', lambda: pytest.fail('library touched'))
    monkeypatch.setattr(_lib, 'require_gpu',
                        lambda: pytest.fail('device touched'))
    ok = resample.Resampler(16000, 10000)
    assert (ok.up, ok.down, ok.Hh, ok.taps.shape) == (5, 8, 80, (161,))
    assert ok.taps.dtype == np.float32 and ok.taps64.dtype == np.float64
    resample.Resampler(1024, 1, half_width=32, beta=0)
    resample.Resampler(1, 1024, half_width=1, beta=20)
    for args, kw in (((0, 8000), {}), ((8000, -1), {}), ((8000.0, 16000), {}),
                     ((True, 16000), {}), (('a', 16000), {}),
                     ((1025, 1), {}), ((1, 1025), {}), ((1031, 1033), {}),
                     ((16000, 10000), dict(half_width=0)),
                     ((16000, 10000), dict(half_width=33)),
                     ((16000, 10000), dict(half_width=2.0)),
                     ((16000, 10000), dict(beta=-0.1)),
                     ((16000, 10000), dict(beta=20.5)),
                     ((16000, 10000), dict(beta=float('nan'))),
                     ((16000, 10000), dict(beta='5'))):
        with pytest.raises(ValueError):
            resample.Resampler(*args, **kw)
    # 2 Hh + 1 <= 65537 holds for every half_width <= 32 and ratio <= 1024
    assert 2 * 32 * 1024 + 1 == resample.TAPS_MAX
    x = np.zeros((2, 64), np.float32)
    for bad in ([64], [64, 65], [-1, 3], [1.0, 2.0], [True, False]):
        with pytest.raises(ValueError):
            ok(x, bad)
        with pytest.raises(ValueError):
            ok.reference(x, bad)
    with pytest.raises(ValueError):
        ok(np.zeros((2, 3, 4), np.float32))
    with pytest.raises(ValueError):
        ok(np.zeros(16, np.int32))
    with pytest.raises(ValueError):            # B <= 65535
        ok(np.broadcast_to(np.float32(0), (65536, 4)))
    with pytest.raises(ValueError):            # T <= 2^30
        ok(np.broadcast_to(np.float32(0), (1, 2 ** 30 + 1)))
    with pytest.raises(ValueError):            # out_length(T) <= 2^30
        resample.Resampler(1, 2)(np.broadcast_to(np.float32(0),
                                                 (1, 2 ** 29 + 1)))
    with pytest.raises(ValueError):            # out: a device tensor
        ok(x, out=np.zeros((2, 40), np.float32))


def test_settings_round_trip():
    from wavenet import resample
    rs = resample.Resampler(44100, 10000, half_width=7, beta=6.5)
    assert rs.settings() == {'rate_in': 44100, 'rate_out': 10000,
                             'half_width': 7, 'beta': 6.5}
    again = resample.Resampler.from_settings(rs.settings())
    assert again.settings() == rs.settings()
    assert np.array_equal(again.taps, rs.taps) and \
        np.array_equal(again.table, rs.table)
    for bad in ({}, dict(rs.settings(), more=1), 'x',
                dict(rs.settings(), half_width=40)):
        with pytest.raises(ValueError):
            resample.Resampler.from_settings(bad)
    assert rs.out_length(0) == 0 and rs.out_length(1) == 1
    assert rs.out_length(441) == 100 and rs.out_length(442) == 101


# -------------------------------------------------------------------- taps
def test_taps_at_equal_rates_are_an_impulse_up_to_rounding():
    # (firwin refuses the cutoff 1 / m = 1 and resample_poly copies instead of
    # designing a filter; the rule's design stays defined)
    from wavenet import resample
    rs = resample.Resampler(8000, 8000)
    assert (rs.up, rs.down, rs.Hh) == (1, 1, 10)
    side = np.delete(rs.taps64, 10)
    assert abs(rs.taps64[10] - 1.0) < 1e-12 and np.abs(side).max() < 1e-15


@pytest.mark.parametrize('up,down', [r for r in RATIOS if r != (1, 1)] +
                         [(1, 1000), (1000, 1001)])
@pytest.mark.parametrize('half_width,beta', [(10, 5.0), (1, 0.0), (32, 12.5)])
def test_taps_are_resample_polys_design(up, down, half_width, beta):
    from scipy import signal
    from wavenet import resample
    rs = resample.Resampler(*_rates(up, down), half_width=half_width,
                            beta=beta)
    m = max(up, down)
    want = signal.firwin(2 * half_width * m + 1, 1.0 / m,
                         window=('kaiser', beta)) * up
    # relative to the largest tap (a tap at a zero crossing of the sinc is
    # 1e-17 of it and has no relative precision of its own)
    assert np.abs(rs.taps64 - want).max() <= 1e-12 * np.abs(want).max()
    assert np.array_equal(rs.taps, rs.taps64.astype(np.float32))
    # the device's table: phase r holds the taps r, r + up, ...
    assert rs.LPS % 2 == 1 and rs.table.shape == (up, rs.LPS)
    for r in range(up):
        row = rs.taps[r::up]
        assert np.array_equal(rs.table[r, :len(row)], row)
        assert not rs.table[r, len(row):].any()


# ---------------------------------------------------- the float64 restatement
@pytest.mark.parametrize('up,down', RATIOS)
def test_restatement_agrees_with_resample_poly(up, down):
    from scipy import signal
    from wavenet import resample
    rs = resample.Resampler(*_rates(up, down))
    for n in (1, 7, 500, 1237):
        x = _signal(n, n).astype(np.float64)
        got = R.resample64(x, up, down, rs.taps64)
        # (resample_poly multiplies a given window by `up` itself)
        want = signal.resample_poly(x, up, down, window=rs.taps64 / up)
        assert got.shape == want.shape == (rs.out_length(n),)
        assert np.abs(got - want).max() <= 1e-12 * max(1.0,
                                                       np.abs(want).max())


@pytest.mark.parametrize('up,down', [r for r in RATIOS if r != (1, 1)] +
                         [(1, 1000), (1000, 1001)])
@pytest.mark.parametrize('half_width', [1, 10])
def test_rule_agrees_with_the_restatement(up, down, half_width):
    from wavenet import resample
    rs = resample.Resampler(*_rates(up, down), half_width=half_width)
    n = 3 * max(up, down) // up + 200 if up < 100 else 40
    x = _signal(n, 3)
    got = rs.reference(x)
    tol, y64 = R.bound(x, up, down, rs.taps,
                       [got, R.reversed_order32(x, up, down, rs.taps)])
    assert got.dtype == np.float32 and got.shape == y64.shape
    err = float(np.abs(got - y64).max())
    print('resample %d/%d hw %d: error %.3e, bound %.3e' %
          (up, down, half_width, err, tol))
    assert err <= tol


def test_equal_rates_copy():
    from wavenet import resample
    rs = resample.Resampler(16000, 16000)
    x = _signal(50)
    x[7] = np.nan
    x[9] = -0.0
    got = rs.reference(np.stack([x, x]), [50, 20])
    assert np.array_equal(got[0].view(np.int32), x.view(np.int32))
    assert np.array_equal(got[1, :20].view(np.int32), x[:20].view(np.int32))
    assert not got[1, 20:].view(np.int32).any()


def test_reference_lengths_batches_and_nan():
    from wavenet import resample
    rs = resample.Resampler(16000, 10000)
    x = np.stack([_signal(300, s) for s in range(4)])
    n = [300, 0, 1, 137]
    got = rs.reference(x, n)
    assert got.shape == (4, rs.out_length(300))
    for b in range(4):
        no = rs.out_length(n[b])
        alone = rs.reference(x[b, :n[b]]) if n[b] else np.zeros(0, np.float32)
        assert np.array_equal(got[b, :no].view(np.int32),
                              alone.view(np.int32))
        assert not got[b, no:].view(np.int32).any()
    # poison behind n[b] is never read
    y = x.copy()
    for b in range(4):
        y[b, n[b]:] = np.nan
    assert np.array_equal(rs.reference(y, n).view(np.int32),
                          got.view(np.int32))
    # a NaN reaches exactly the outputs whose taps cover it
    z = x[0].copy()
    z[100] = np.nan
    bad = np.nonzero(~np.isfinite(rs.reference(z)))[0]
    assert np.array_equal(bad, R.reach(100, 300, 5, 8, 80)) and len(bad) == 20


# ----------------------------------------------------------------- bindings
def _declarations(header):
    src = open(os.path.join(ROOT, 'include', header)).read()
    src = re.sub(r'/\*.*?\*/', ' ', src, flags=re.S)
    return {m.group(2): (m.group(1), [' '.join(p.split())
                                      for p in m.group(3).split(',')])
            for m in re.finditer(
                r'\b(int|long)\s+(wn_\w+)\s*\(([^)]*)\)\s*;', src)}


def _tables(_lib):
    return {k: v for k, v in vars(_lib).items() if k.endswith('SIGNATURES')}


def test_binding_table_matches_its_header():
    from wavenet import _lib
    decl = _declarations(HEADER)
    assert set(decl) == {'wn_resample_tile', 'wn_resample'}
    assert set(_lib.RESAMPLE_SIGNATURES) == set(decl)
    ctype = {'int': _lib.c_int, 'long': _lib.c_long, 'float': _lib.c_float,
             'double': _lib.c_double}
    for name, (res, params) in decl.items():
        params = [p for p in params if p != 'void']
        want = [_lib.P if '*' in p else ctype[p.split()[0]] for p in params]
        assert _lib.RESAMPLE_SIGNATURES[name] == (ctype[res], want), name
    for path in glob.glob(os.path.join(ROOT, 'include', '*.h')):
        other = os.path.basename(path)
        if other != HEADER:
            assert not set(decl) & set(_declarations(other)), other
    for name, table in _tables(_lib).items():
        if name != 'RESAMPLE_SIGNATURES':
            assert not set(decl) & set(table), name


def test_load_binds_the_table(hip_lib):
    from wavenet import _lib
    for name, (res, args) in _lib.RESAMPLE_SIGNATURES.items():
        fn = getattr(hip_lib, name)
        assert fn.restype is res and fn.argtypes == args, name


def test_every_writing_entry_of_the_header_is_guarded():
    import test_gpu_guard_resample as tg
    w = {k: [p for p in v[1] if '*' in p and not p.startswith('const ')
             and not re.search(r'\bstream$', p)]
         for k, v in _declarations(HEADER).items()}
    w = {k: v for k, v in w.items() if v}
    assert w == {'wn_resample': ['float* out']}
    assert set(tg.ENTRIES) == set(w)


OK, BAD_SHAPE, MISALIGNED, NULL = 0, -1, -3, -5


def test_the_entrys_own_checks(hip_lib):
    """Every refusal comes back before any launch (no device here)."""
    import ctypes
    from wavenet import resample
    assert hip_lib.wn_resample_tile() == resample.Resampler.tile() == 256
    buf = (ctypes.c_double * 8192)()
    a = ctypes.addressof(buf)
    fn = hip_lib.wn_resample
    # x, ld_x, lengths, B, T, up, down, Hh, tab, out, ld_out, stream
    good = [a, 600, None, 2, 600, 5, 8, 80, a + 16384, a + 32768, 375, None]

    def with_(i, v):
        g = list(good)
        g[i] = v
        return g
    for i in (0, 8, 9):
        assert fn(*with_(i, None)) == NULL
    for i, v in ((1, 599), (3, 0), (3, 65536), (4, 0), (4, 2 ** 30 + 1),
                 (5, 0), (5, 1025), (5, 4), (6, 0), (6, 1025), (6, 10),
                 (7, -1), (7, 32769), (10, 374)):
        assert fn(*with_(i, v)) == BAD_SHAPE, (i, v)
    # out_length(T) <= 2^30
    assert fn(a, 2 ** 30, None, 1, 2 ** 30, 2, 1, 20, a, a + 2 ** 33,
              2 ** 31, None) == BAD_SHAPE
    for i in (0, 2, 8, 9):
        assert fn(*with_(i, a + 32768 + 4096 + 2)) == MISALIGNED
    assert fn(*with_(9, a + 400)) == BAD_SHAPE        # out overlaps x
