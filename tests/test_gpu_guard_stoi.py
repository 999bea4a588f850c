"""Guard bands (tests/guard.py) around the operands of the entry of
include/wavenet_stoi.h that writes through a pointer: wn_stoi's four launches
read and write nothing outside them -- poisoned margins round both signals
(padded rows: the gap columns belong to the band), the lengths, the window, the
basis, the scratch and the four outputs; what lies behind n[b] INSIDE the
signals is poison too, so no output depends on it.  tests/test_stoi_host.py
holds ENTRIES against the header."""
import numpy as np
import pytest
import torch

import guard
import stoi_ref as S

pytestmark = pytest.mark.gpu

# the entries of wavenet_stoi.h that write through a pointer
ENTRIES = ('wn_stoi',)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _problem(lengths_of):
    """Clips at 10 kHz: (generated, original, n) from fixtures cut or padded
    to the given lengths (None: the fixture's own)."""
    clips = []
    for M, n in lengths_of:
        x = S.fixture(M, 10000)
        y = S.degraded(x, 0.2, seed=M)
        n = len(x) if n is None else n
        clips.append((y[:n], x[:n], n))
    T = max(c[2] for c in clips)
    g = np.full((len(clips), T), np.nan, np.float32)   # poison behind n[b]
    o = np.full((len(clips), T), np.nan, np.float32)
    for b, (y, x, n) in enumerate(clips):
        g[b, :n], o[b, :n] = y, x
    return g, o, np.array([c[2] for c in clips], np.int32)


# (clips as (fixture M, length), ld - T of generated and original, skew)
CASES = [(((65, None), (31, None), (31, 255), (31, 0), (29, None)), 3, 5, 0),
         (((30, None), (31, 256)), 0, 0, 4),
         (((31, 200), (31, 1)), 1, 0, 4)]


@pytest.mark.parametrize('clips,gap_g,gap_o,skew', CASES)
def test_stoi_stays_inside_its_operands(hip_lib, clips, gap_g, gap_o, skew):
    from wavenet import stoi
    meter = stoi.Stoi(10000)
    g, o, n = _problem(clips)
    B, T = g.shape
    clean_g, clean_o = np.nan_to_num(g), np.nan_to_num(o)
    want = [t.cpu() for t in meter(clean_g, clean_o, n)]
    words = hip_lib.wn_stoi_scratch_bytes(B, T) // 8
    ar = guard.Arena('cuda')
    ar.place('gen', g, torch.float32, ld=T + gap_g if gap_g else None,
             skew_bytes=skew)
    ar.place('org', o, torch.float32, ld=T + gap_o if gap_o else None,
             skew_bytes=skew)
    ar.place('lengths', n, torch.int32, fill=(T, 0), skew_bytes=skew)
    ar.place('window', meter.window, torch.float32, skew_bytes=skew)
    ar.place('basis', meter.basis, torch.float32, skew_bytes=skew)
    ar.place('scratch', (words,), torch.float64, role='out')
    ar.place('stoi_sum', (B,), torch.float64, role='out')
    ar.place('estoi_sum', (B,), torch.float64, role='out')
    ar.place('segments', (B,), torch.int32, role='out', skew_bytes=skew)
    ar.place('kept', (B,), torch.int32, role='out', skew_bytes=skew)

    def run():
        code = hip_lib.wn_stoi(
            ar.ptr('gen'), T + gap_g, ar.ptr('org'), T + gap_o,
            ar.ptr('lengths'), B, T, ar.ptr('window'), ar.ptr('basis'),
            ar.ptr('scratch'), ar.ptr('stoi_sum'), ar.ptr('estoi_sum'),
            ar.ptr('segments'), ar.ptr('kept'), _stream())
        assert code == 0, code
    bits = guard.read_check(ar, run)
    ar.check()
    for name, w in zip(('stoi_sum', 'estoi_sum', 'segments', 'kept'), want):
        wide = w.dtype == torch.float64
        got = bits[name].cpu()
        assert torch.equal(got, w.view(torch.int64) if wide else w), name


def test_stoi_without_lengths(hip_lib):
    from wavenet import stoi
    meter = stoi.Stoi(10000)
    x = S.fixture(31, 10000)
    y = S.degraded(x, 0.2, seed=31)
    g, o = np.stack([y, x]), np.stack([x, x])
    B, T = g.shape
    want = [t.cpu() for t in meter(g, o)]
    ar = guard.Arena('cuda')
    ar.place('gen', g, torch.float32, ld=T + 2, skew_bytes=4)
    ar.place('org', o, torch.float32, ld=T + 6)
    ar.place('window', meter.window, torch.float32)
    ar.place('basis', meter.basis, torch.float32)
    ar.place('scratch', (hip_lib.wn_stoi_scratch_bytes(B, T) // 8,),
             torch.float64, role='out')
    ar.place('stoi_sum', (B,), torch.float64, role='out')
    ar.place('estoi_sum', (B,), torch.float64, role='out')
    ar.place('segments', (B,), torch.int32, role='out')
    ar.place('kept', (B,), torch.int32, role='out')

    def run():
        code = hip_lib.wn_stoi(
            ar.ptr('gen'), T + 2, ar.ptr('org'), T + 6, None, B, T,
            ar.ptr('window'), ar.ptr('basis'), ar.ptr('scratch'),
            ar.ptr('stoi_sum'), ar.ptr('estoi_sum'), ar.ptr('segments'),
            ar.ptr('kept'), _stream())
        assert code == 0, code
    bits = guard.read_check(ar, run)
    ar.check()
    for name, w in zip(('stoi_sum', 'estoi_sum', 'segments', 'kept'), want):
        got = bits[name].cpu()
        assert torch.equal(got, w.view(torch.int64)
                           if w.dtype == torch.float64 else w), name
    assert bits['kept'].tolist() == [31, 31]
