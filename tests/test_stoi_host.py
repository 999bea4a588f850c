"""wavenet/stoi.py without a device: limits, the band edges, the float64
restatement (tests/stoi_ref.py) against closed forms, the fixtures' distance
from the keep threshold, the numpy rule against the restatement, StoiSums, the
binding table against include/wavenet_stoi.h and evaluate.py's refusals."""
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import stoi_ref as S
from util import ROOT

HEADER = 'wavenet_stoi.h'
# (M, rate) of every fixture the GPU tests use
FIXTURES = [(29, 16000), (30, 16000), (31, 16000), (65, 16000), (31, 10000)]


# ------------------------------------------------------------------ limits
def test_limits_come_before_the_library(monkeypatch):
    from wavenet import _lib, stoi
    monkeypatch.setattr(_lib, 'load', lambda: pytest.fail('library touched'))
    monkeypatch.setattr(_lib, 'require_gpu',
                        lambda: pytest.fail('device touched'))
    assert stoi.Stoi(10000).resampler is None
    m = stoi.Stoi(16000)
    assert (m.resampler.up, m.resampler.down) == (5, 8)
    assert stoi.Stoi(44100).resampler.down == 441
    for bad in (0, -16000, 16000.0, True, '16000', 10250001):
        with pytest.raises(ValueError):
            stoi.Stoi(bad)
    x = np.zeros((2, 600), np.float32)
    with pytest.raises(ValueError):
        m(x, x[:, :599])
    with pytest.raises(ValueError):
        m(x, x, [600, 601])
    with pytest.raises(ValueError):
        m(x, x, [600])
    with pytest.raises(ValueError):
        m(x.astype(np.int32), x)
    big = np.broadcast_to(np.float32(0), (65536, 4))
    with pytest.raises(ValueError):
        m(big, big)
    assert m.settings() == {'sample_rate': 16000, 'half_width': 10,
                            'beta': 5.0}
    again = stoi.Stoi.from_settings(m.settings())
    assert again.settings() == m.settings() and \
        np.array_equal(again.resampler.taps, m.resampler.taps)
    for bad in ({}, dict(m.settings(), more=1), 'x'):
        with pytest.raises(ValueError):
            stoi.Stoi.from_settings(bad)


def test_band_edges_window_and_constants(hip_lib):
    from wavenet import stoi
    assert stoi.band_edges().tolist() == S.L + [219]
    assert S.U == S.L[1:] + [219]
    assert [hip_lib.wn_stoi_band_edge(i) for i in range(16)] == S.L + [219]
    assert hip_lib.wn_stoi_band_edge(-1) == hip_lib.wn_stoi_band_edge(16) == -1
    # the closest edge to a rounding tie is 0.01797 of a bin away from it
    # (34.482 -> 34): six orders above float64's rounding of the formula
    b = np.arange(16)
    exact = 150.0 * 2.0 ** (b / 3.0) * 2.0 ** (-1.0 / 6.0) * 512 / 10000
    assert np.abs(np.abs(exact - np.round(exact)) - 0.5).min() > 0.0179
    assert np.array_equal(stoi.window(), S.window64().astype(np.float32))
    assert stoi.window()[0] > 0 and stoi.window()[-1] > 0
    assert stoi.CLIP == S.C == 10 ** 0.75 and stoi.EPS == S.EPS == 2.0 ** -52
    assert float(stoi.RANGE) == float(np.float32(1e-4))
    assert stoi.frames_of(np.array([0, 255, 256, 383, 384])).tolist() == \
        [0, 0, 1, 1, 2]


# --------------------------------------------- the restatement, closed forms
def test_restatement_closed_forms():
    x = S.fixture(65, 10000)
    r = S.stoi64(x, x)
    assert r['kept'] == 65 and r['segments'] == 36
    assert abs(r['stoi'] - 1) < 1e-12 and abs(r['estoi'] - 1) < 1e-12
    for g in (0.3, 3.0):
        r = S.stoi64(g * x.astype(np.float64), x)
        assert abs(r['stoi'] - 1) < 1e-9 and abs(r['estoi'] - 1) < 1e-9
    st, es = [], []
    for sigma in (0.01, 0.03, 0.1, 0.3, 1.0):
        r = S.stoi64(S.degraded(x, sigma), x)
        st.append(r['stoi'])
        es.append(r['estoi'])
    print('stoi', st, 'estoi', es)
    assert all(a > b for a, b in zip(st, st[1:])), st
    assert all(a > b for a, b in zip(es, es[1:])), es
    assert 1 > st[0] and 1 > es[0]


def test_restatement_skips():
    x = S.fixture(31, 10000)
    for clip in (np.zeros(4000, np.float32), x[:255], S.fixture(29, 10000)):
        r = S.stoi64(clip, clip)
        assert r['segments'] == 0 and r['stoi_sum'] == 0.0 and \
            r['estoi_sum'] == 0.0 and r['stoi'] is None
    assert S.stoi64(x[:255], x[:255])['frames'] == 0
    assert S.stoi64(np.zeros(4000), np.zeros(4000))['kept'] == 0
    assert S.stoi64(S.fixture(29, 10000), S.fixture(29, 10000))['kept'] == 29
    # the corpus mean leaves them out
    rs = [S.stoi64(x, x), S.stoi64(x[:255], x[:255])]
    c = S.corpus(rs)
    assert (c['clips'], c['skipped_clips'], c['segments']) == (1, 1, 2)


@pytest.mark.parametrize('M,rate', FIXTURES)
def test_fixtures_are_decisive(M, rate):
    from wavenet import stoi
    x = S.fixture(M, rate)
    meter = stoi.Stoi(rate)
    r = S.stoi64(x, x, meter.resampler)
    assert r['kept'] == M and S.decisive(r['margin'])
    k = np.nonzero(r['keep'])[0]
    # removed frames at the start, in the middle and at the end
    assert k[0] > 0 and k[-1] < r['frames'] - 1 and \
        len(k) < k[-1] - k[0] + 1
    print('fixture M %d at %d Hz: %d frames, closest margin %.3f'
          % (M, rate, r['frames'],
             np.abs(np.log(r['margin'][r['margin'] > 0])).min()))


# ------------------------------------------------- the numpy rule of the package
@pytest.mark.parametrize('M,rate', [(31, 16000), (31, 10000)])
def test_rule_agrees_with_the_restatement(M, rate):
    from wavenet import stoi
    x = S.fixture(M, rate)
    y = S.degraded(x, 0.1)
    meter = stoi.Stoi(rate)
    got = meter.reference(y, x)
    want = S.stoi64(y, x, meter.resampler)
    assert (got['kept'], got['segments'], got['frames']) == \
        (want['kept'], want['segments'], want['frames'])
    alt = S.alt32(y, x, meter.resampler, want['keep'])
    for key, other in (('stoi', alt[0]), ('estoi', alt[1])):
        mine = got[key + '_sum'] / got['segments']
        tol = S.bound(want[key], [mine, other])
        print('%s: reference %.9f, restatement %.9f, bound %.3e'
              % (key, mine, want[key], tol))
        assert abs(mine - want[key]) <= tol
    # skipped clips
    for clip in (np.zeros(5000, np.float32), x[:300], S.fixture(29, rate)):
        r = meter.reference(clip, clip)
        assert r['segments'] == 0 and r['stoi_sum'] == 0.0 and \
            r['estoi_sum'] == 0.0
    same = meter.reference(x, x)
    assert abs(same['stoi_sum'] / same['segments'] - 1) < 1e-12 and \
        abs(same['estoi_sum'] / same['segments'] - 1) < 1e-12


def test_sums_cat_and_summary():
    import torch
    from wavenet import stoi
    a = stoi.StoiSums(torch.tensor([1.5, 0.0], dtype=torch.float64),
                      torch.tensor([1.0, 0.0], dtype=torch.float64),
                      torch.tensor([2, 0], dtype=torch.int32),
                      torch.tensor([31, 4], dtype=torch.int32), [40, 9])
    b = stoi.StoiSums(torch.tensor([0.5], dtype=torch.float64),
                      torch.tensor([-0.25], dtype=torch.float64),
                      torch.tensor([1], dtype=torch.int32),
                      torch.tensor([30], dtype=torch.int32), [33])
    s = stoi.StoiSums.cat([a, b]).summary()
    assert s == {'stoi': (0.75 + 0.5) / 2, 'estoi': (0.5 - 0.25) / 2,
                 'clips': 2, 'skipped_clips': 1, 'segments': 3,
                 'kept_frames': 65, 'frames': 82, 'sample_rate': 10000}
    with pytest.raises(ValueError):
        stoi.StoiSums.cat([])
    none = stoi.StoiSums(*(t[1:] for t in a), frames=[9])
    with pytest.raises(ValueError, match='no clip'):
        none.summary()


# ----------------------------------------------------------------- bindings
def _declarations(header):
    src = open(os.path.join(ROOT, 'include', header)).read()
    src = re.sub(r'/\*.*?\*/', ' ', src, flags=re.S)
    return {m.group(2): (m.group(1), [' '.join(p.split())
                                      for p in m.group(3).split(',')])
            for m in re.finditer(
                r'\b(int|long)\s+(wn_\w+)\s*\(([^)]*)\)\s*;', src)}


def test_binding_table_matches_its_header():
    from wavenet import _lib
    decl = _declarations(HEADER)
    assert set(decl) == {'wn_stoi_band_edge', 'wn_stoi_scratch_bytes',
                         'wn_stoi'}
    assert set(_lib.STOI_SIGNATURES) == set(decl)
    ctype = {'int': _lib.c_int, 'long': _lib.c_long, 'float': _lib.c_float,
             'double': _lib.c_double}
    for name, (res, params) in decl.items():
        params = [p for p in params if p != 'void']
        want = [_lib.P if '*' in p else ctype[p.split()[0]] for p in params]
        assert _lib.STOI_SIGNATURES[name] == (ctype[res], want), name
    for path in glob.glob(os.path.join(ROOT, 'include', '*.h')):
        other = os.path.basename(path)
        if other != HEADER:
            assert not set(decl) & set(_declarations(other)), other
    for name, table in vars(_lib).items():
        if name.endswith('SIGNATURES') and name != 'STOI_SIGNATURES':
            assert not set(decl) & set(table), name


def test_load_binds_the_table(hip_lib):
    from wavenet import _lib
    for name, (res, args) in _lib.STOI_SIGNATURES.items():
        fn = getattr(hip_lib, name)
        assert fn.restype is res and fn.argtypes == args, name


def test_every_writing_entry_of_the_header_is_guarded():
    import test_gpu_guard_stoi as tg
    w = {k: [p for p in v[1] if '*' in p and not p.startswith('const ')
             and not re.search(r'\bstream$', p)]
         for k, v in _declarations(HEADER).items()}
    w = {k: v for k, v in w.items() if v}
    assert w == {'wn_stoi': ['void* scratch', 'double* stoi_sum',
                             'double* estoi_sum', 'int32_t* segments',
                             'int32_t* kept']}
    assert set(tg.ENTRIES) == set(w)


OK, BAD_SHAPE, MISALIGNED, NULL = 0, -1, -3, -5


def test_the_entries_own_checks(hip_lib):
    """Every refusal comes back before any launch (no device here)."""
    import ctypes
    sb = hip_lib.wn_stoi_scratch_bytes
    # 4000 samples: 30 frames, 1 segment
    assert sb(1, 4000) == 16 + 4 * 30 * 32 and sb(3, 255) == 3 * (16 + 128)
    assert sb(2, 4096 + 128) == 2 * (16 * 3 + 4 * 32 * 32)
    for B, T in ((0, 4000), (65536, 4000), (1, 0), (1, 2 ** 30 + 1)):
        assert sb(B, T) == BAD_SHAPE
    buf = (ctypes.c_double * 8192)()
    a = ctypes.addressof(buf)
    fn = hip_lib.wn_stoi
    # gen, ld, org, ld, lengths, B, T, window, basis, scratch, stoi_sum,
    # estoi_sum, segments, kept, stream
    good = [a, 600, a + 8192, 600, None, 2, 600, a, a, a, a, a, a, a, None]

    def with_(i, v):
        g = list(good)
        g[i] = v
        return g
    for i in (0, 2, 7, 8, 9, 10, 11, 12, 13):
        assert fn(*with_(i, None)) == NULL
    for i, v in ((1, 599), (3, 599), (5, 0), (5, 65536), (6, 0),
                 (6, 2 ** 30 + 1)):
        assert fn(*with_(i, v)) == BAD_SHAPE, (i, v)
    for i in (0, 2, 4, 7, 8, 12, 13):
        assert fn(*with_(i, a + 2)) == MISALIGNED, i
    for i in (9, 10, 11):
        assert fn(*with_(i, a + 4)) == MISALIGNED, i


# ------------------------------------------------------------- evaluate.py
@pytest.mark.parametrize('argv,words', [
    (['--synthesis_stoi', 'true'], ('--synthesis_stoi', '--synthesis true')),
    (['--synthesis_stoi', 'false'], ('--synthesis_stoi', '--synthesis true')),
])
def test_evaluate_refuses(argv, words):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'evaluate.py'),
                        'ck', '--data_dir', 'd'] + argv, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=120)
    out = p.stdout.decode()
    assert p.returncode == 2, out
    for w in words:
        assert w in out, out


def test_evaluate_docstring_has_its_paragraph():
    src = open(os.path.join(ROOT, 'evaluate.py')).read()
    assert '"synthesis_stoi":' in src and 'resample_poly' in src
