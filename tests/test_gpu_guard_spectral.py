"""Guard bands (tests/guard.py) around the operands of the entries of
include/wavenet_spectral.h that write through a pointer: wn_stft_distance and
wn_cepstral_distance read and write nothing outside them -- poisoned margins
round both signals (padded rows, ld_gen != ld_org: the gap columns belong to
the band), the lengths, the tables, the three outputs and the scratch; and
what lies behind n[b] INSIDE a signal is poison too, so no output depends on
it.  tests/test_spectral_host.py holds ENTRIES against the header, the rule
tests/test_guard_host.py keeps for wavenet_hip.h."""
import numpy as np
import pytest
import torch

import guard
import stft_ref as R

pytestmark = pytest.mark.gpu

# the entries of wavenet_spectral.h that write through a pointer
ENTRIES = ('wn_stft_distance', 'wn_cepstral_distance')

# (shape of stft_ref.SHAPES, ld_gen - T, ld_org - T): staged and memory paths
CASES = [('tiles', 3, 0), ('oddhop', 0, 7), ('r512', 5, 9),
         ('r2048', 1, 2), ('e2048m', 2, 5), ('e1024s', 0, 0)]


def _lengths(name):
    T, lengths = R.SHAPES[name][3:]
    # (without lengths of its own a shape gets ragged ones here)
    return [T, T - 1, T // 2, 1] if lengths is None else list(lengths)


def _build(name, gap_g, gap_o, skew=0, with_lengths=True):
    from wavenet import spectral
    n_fft, hop, win, T, _ = R.SHAPES[name]
    g, o = R.make_pair(name)
    n = _lengths(name) if with_lengths else None
    if n is not None:
        for b in range(4):                 # poison behind the clip's end
            g[b, n[b]:] = np.nan
            o[b, n[b]:] = np.nan
    spec = spectral.StftDistance(((n_fft, hop, win),))._specs[0]
    window, basis, _ = spec.device_tables(torch.device('cuda'))
    ar = guard.Arena('cuda')
    ar.place('gen', g, torch.float32, ld=T + gap_g if gap_g else None,
             skew_bytes=skew)
    ar.place('org', o, torch.float32, ld=T + gap_o if gap_o else None,
             skew_bytes=skew)
    if n is not None:
        # (band values that are lengths themselves: T, then 1)
        ar.place('lengths', np.asarray(n, np.int32), torch.int32,
                 fill=(T, 1), skew_bytes=skew)
    ar.place('window', window.cpu(), torch.float32, skew_bytes=skew)
    # (bands of a tile of basis rows, not of the whole table)
    ar.place('basis', basis.cpu(), torch.float32, tile_ld=64)
    for k in R.OUTPUTS:
        ar.place(k, (4,), torch.float64, role='out')
    parts = 3 * 4 * -(-(-(-T // hop)) // 32)
    ar.place('partials', (parts,), torch.float64, role='out')

    def run(lib):
        assert lib.wn_stft_distance_partials(4, T, hop) == parts
        code = lib.wn_stft_distance(
            ar.ptr('gen'), T + gap_g, ar.ptr('org'), T + gap_o, 4, T,
            ar.ptr('lengths' if n is not None else None), ar.ptr('window'),
            ar.ptr('basis'), n_fft, hop, n_fft // 2 + 1, R.FLOOR,
            ar.ptr('sc_num'), ar.ptr('sc_den'), ar.ptr('log_sum'),
            ar.ptr('partials'), torch.cuda.current_stream().cuda_stream)
        assert code == 0, code
    return ar, run


def _clean(name, with_lengths=True):
    """The bits of the three outputs from clean, contiguous signals."""
    from wavenet import spectral
    n_fft, hop, win = R.SHAPES[name][:3]
    g, o = R.make_pair(name)
    got = spectral.StftDistance(((n_fft, hop, win),))(
        g, o, _lengths(name) if with_lengths else None)
    return {k: t.cpu().view(torch.int64)[0] for k, t in zip(R.OUTPUTS, got)}


@pytest.mark.parametrize('name,gap_g,gap_o', CASES)
def test_stft_distance_stays_inside_its_operands(hip_lib, name, gap_g, gap_o):
    ar, run = _build(name, gap_g, gap_o)
    run(hip_lib)
    torch.cuda.synchronize()
    ar.check()
    bits = guard.read_check(ar, lambda: run(hip_lib))
    ar.check()
    # (every word of every output and of the scratch was written)
    for key, b in bits.items():
        assert not (b == guard._signed(guard.BODY64, 64)).any(), key
    # poison behind n[b] and in the gaps reached no output
    want = _clean(name)
    for key in R.OUTPUTS:
        assert torch.equal(bits[key].cpu(), want[key]), key


def test_stft_distance_without_lengths(hip_lib):
    ar, run = _build('r512', 4, 1, with_lengths=False)
    bits = guard.read_check(ar, lambda: run(hip_lib))
    ar.check()
    want = _clean('r512', with_lengths=False)
    for key in R.OUTPUTS:
        assert torch.equal(bits[key].cpu(), want[key]), key


@pytest.mark.parametrize('name,gap_g,gap_o', [('r512', 5, 9), ('e2048m', 2, 5)])
def test_stft_distance_four_bytes_off_alignment(hip_lib, name, gap_g, gap_o):
    ar, run = _build(name, gap_g, gap_o, skew=4)
    assert ar.ptr('gen') % 16 == 4 and ar.ptr('window') % 16 == 4
    got = guard.read_check(ar, lambda: run(hip_lib))
    ar.check()
    want = _clean(name)
    for key in R.OUTPUTS:
        assert torch.equal(got[key].cpu(), want[key]), key


@pytest.mark.parametrize('C,K,F', [(80, 13, 65), (5, 4, 64), (128, 64, 63),
                                   (3, 1, 200)])
def test_cepstral_distance_stays_inside_its_operands(hip_lib, C, K, F):
    from wavenet import spectral
    a, b = R.logmel_pair(7 * C + F, 3, F, C)
    nf = np.array([F, (F + 1) // 2, 0], np.int32)
    want = spectral.cepstral_distance(a, b, nf, K).cpu().view(torch.int64)
    for i in range(3):                     # poison behind the real frames
        a[i, nf[i]:] = np.nan
        b[i, nf[i]:] = np.nan
    ar = guard.Arena('cuda')
    ar.place('a', a, torch.float32, skew_bytes=4)
    ar.place('b', b, torch.float32, skew_bytes=4)
    ar.place('nframes', nf, torch.int32, fill=(F, 0), skew_bytes=4)
    ar.place('dct', spectral.dct_table(C, K), torch.float64)
    ar.place('mcd_sum', (3,), torch.float64, role='out')
    ar.place('partials', (hip_lib.wn_cepstral_distance_partials(3, F),),
             torch.float64, role='out')

    def run():
        code = hip_lib.wn_cepstral_distance(
            ar.ptr('a'), ar.ptr('b'), 3, F, C, ar.ptr('nframes'),
            ar.ptr('dct'), K, ar.ptr('mcd_sum'), ar.ptr('partials'),
            torch.cuda.current_stream().cuda_stream)
        assert code == 0, code
    bits = guard.read_check(ar, run)
    ar.check()
    for key, v in bits.items():
        assert not (v == guard._signed(guard.BODY64, 64)).any(), key
    assert torch.equal(bits['mcd_sum'].cpu(), want)
