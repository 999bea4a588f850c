"""wn_stft_distance and wn_cepstral_distance (include/wavenet_spectral.h,
wavenet/spectral.py) on the device against the float64 restatement of
tests/stft_ref.py, at every kernel shape of stft_ref.SHAPES -- a partial last
tile, idle waves, an odd hop, no overlap, a second tile of two frames, the
three default resolutions, ragged lengths, and a pair of hops either side of
the LDS staging edge at n_fft 2048 and 1024 -- each output of each clip within
stft_ref.rel_tol (4 x the CPU yardstick of its shape) of its own scale; exact
zeros for an equal pair; a clip alone against the same clip at every position
of a batch, bit for bit; padded leading dimensions; a NaN stays in its clip;
lengths=None is lengths=[T] * B."""
import functools

import numpy as np
import pytest
import torch

import stft_ref as R

pytestmark = pytest.mark.gpu


def _dist(name):
    from wavenet import spectral
    return spectral.StftDistance((R.SHAPES[name][:3],))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def _lengths(name):
    T, lengths = R.SHAPES[name][3:]
    return [T] * 4 if lengths is None else list(lengths)


@functools.lru_cache(maxsize=None)
def _want(name):
    """Per clip (sums, scales) of shape `name` in float64, computed once."""
    n_fft, hop, win = R.SHAPES[name][:3]
    g, o = R.make_pair(name)
    out = []
    for b, n in enumerate(_lengths(name)):
        out.append((R.stft_sums(g[b, :n], o[b, :n], n_fft, hop, win),
                    R.scales(g[b, :n], o[b, :n], n_fft, hop, win)))
    return out


@pytest.mark.parametrize('name', sorted(R.SHAPES))
def test_sums_against_the_restatement(hip_lib, name):
    n_fft, hop, win, T, lengths = R.SHAPES[name]
    if name in R.STAGED:
        assert hip_lib.wn_stft_distance_staged(n_fft, hop) == R.STAGED[name]
    g, o = R.make_pair(name)
    got = _dist(name)(g, o, lengths)
    got = [t.cpu().numpy()[0] for t in got]
    for b, (ref, scale) in enumerate(_want(name)):
        for k, out in enumerate(R.OUTPUTS):
            err = abs(got[k][b] - ref[k])
            bound = R.rel_tol(name, out) * scale[k]
            print('%s clip %d %s: %.6e (ref %.6e) err %.2e bound %.2e'
                  % (name, b, out, got[k][b], ref[k], err, bound))
            assert err <= bound, (name, b, out)
    # the metrics of the summary, against the restatement's
    s = _dist(name)(g, o, lengths).summary(_lengths(name))
    want = [R.metrics(g[b, :n], o[b, :n], n_fft, hop, win)
            for b, n in enumerate(_lengths(name))]
    assert s['spectral_convergence'] == pytest.approx(
        np.mean([w[0] for w in want]), rel=1e-5)
    assert s['log_stft_magnitude'] == pytest.approx(
        np.mean([w[1] for w in want]), rel=1e-5)


@pytest.mark.parametrize('name', ['tiles', 'r512', 'r2048', 'e2048m'])
def test_equal_pair_gives_exact_zeros(hip_lib, name):
    _, o = R.make_pair(name)
    num, den, lg = _dist(name)(o, o.copy(), R.SHAPES[name][4])
    assert (_bits(num) == 0).all() and (_bits(lg) == 0).all()   # +0.0
    assert (den.cpu().numpy() > 0).all()


@pytest.mark.parametrize('name', ['tiles', 'r512', 'r2048', 'e1024m'])
def test_a_clip_alone_and_at_every_position_of_a_batch(hip_lib, name):
    g, o = R.make_pair(name)
    n = np.array(_lengths(name))
    dist = _dist(name)
    T = g.shape[1]
    alone = []
    for b in range(4):
        # alone, cut to its own length: T differs, the bits do not
        one = dist(g[b, :n[b]], o[b, :n[b]])
        padded = dist(g[b], o[b], n[b:b + 1])
        for x, y in zip(one, padded):
            assert torch.equal(_bits(x), _bits(y)), (name, b)
        alone.append([_bits(t) for t in one])
    for shift in range(4):
        idx = np.roll(np.arange(4), shift)
        got = [_bits(t) for t in dist(g[idx], o[idx], n[idx])]
        for pos, b in enumerate(idx):
            for k in range(3):
                assert got[k][0, pos] == alone[b][k][0, 0], \
                    (name, shift, pos, k)
    assert T == R.SHAPES[name][3]


def _raw(hip_lib, name, g, o, ld_g, ld_o, lengths):
    """wn_stft_distance itself, clip b at + b * ld: int64 bits [3][B]."""
    from wavenet import spectral
    n_fft, hop, win = R.SHAPES[name][:3]
    B, T = g.shape
    dev = torch.device('cuda')
    bufs = []
    for x, ld in ((g, ld_g), (o, ld_o)):
        t = torch.full((B, ld), float('nan'), dtype=torch.float32, device=dev)
        t[:, :T] = torch.from_numpy(x).to(dev)
        bufs.append(t)
    spec = spectral.StftDistance(((n_fft, hop, win),))._specs[0]
    w, basis, _ = spec.device_tables(dev)
    nd = None if lengths is None else \
        torch.tensor(lengths, dtype=torch.int32, device=dev)
    out = torch.empty((3, B), dtype=torch.float64, device=dev)
    parts = torch.empty(hip_lib.wn_stft_distance_partials(B, T, hop),
                        dtype=torch.float64, device=dev)
    code = hip_lib.wn_stft_distance(
        bufs[0].data_ptr(), ld_g, bufs[1].data_ptr(), ld_o, B, T,
        None if nd is None else nd.data_ptr(), w.data_ptr(), basis.data_ptr(),
        n_fft, hop, n_fft // 2 + 1, R.FLOOR, out[0].data_ptr(),
        out[1].data_ptr(), out[2].data_ptr(), parts.data_ptr(),
        torch.cuda.current_stream().cuda_stream)
    assert code == 0, code
    return _bits(out)


@pytest.mark.parametrize('name', ['oddhop', 'r1024', 'e2048m'])
def test_padded_leading_dimensions(hip_lib, name):
    g, o = R.make_pair(name)
    T, lengths = R.SHAPES[name][3:]
    plain = _raw(hip_lib, name, g, o, T, T, lengths)
    skew = _raw(hip_lib, name, g, o, T + 5, T + 12, lengths)
    assert torch.equal(plain, skew)
    api = _dist(name)(g, o, lengths)
    assert torch.equal(plain, torch.stack([_bits(t)[0] for t in api]))


@pytest.mark.parametrize('name', ['r512', 'r2048', 'e1024m'])
def test_a_nan_stays_in_its_clip(hip_lib, name):
    g, o = R.make_pair(name)
    lengths = R.SHAPES[name][4]
    base = [_bits(t) for t in _dist(name)(g, o, lengths)]
    for which in (0, 1):
        bad = [g.copy(), o.copy()]
        bad[which][1, 100] = np.nan
        got = _dist(name)(bad[0], bad[1], lengths)
        for k, t in enumerate(got):
            v = t.cpu().numpy()[0]
            # (sc_den sums the original's magnitudes alone)
            assert np.isnan(v[1]) or (k == 1 and which == 0), (name, which, k)
            keep = [0, 2, 3]
            assert torch.equal(_bits(t)[:, keep], base[k][:, keep])


@pytest.mark.parametrize('name', ['tiles', 'r1024'])
def test_no_lengths_is_full_lengths(hip_lib, name):
    g, o = R.make_pair(name)
    T = g.shape[1]
    a = _dist(name)(g, o)
    b = _dist(name)(g, o, [T] * 4)
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y))


def test_default_resolutions_are_the_single_ones(hip_lib):
    from wavenet import spectral
    g, o = R.make_pair('r1024')
    multi = spectral.StftDistance()
    got = multi(torch.from_numpy(g).cuda(), torch.from_numpy(o).cuda())
    assert got.sc_num.shape == (3, 4) and got.sc_num.dtype == torch.float64
    for r, res in enumerate(multi.resolutions):
        one = spectral.StftDistance((res,))(g, o)
        for x, y in zip(got, one):
            assert torch.equal(_bits(x)[r], _bits(y)[0])
    s = got.summary(4000)
    assert [p['n_fft'] for p in s['per_resolution']] == [1024, 2048, 512]
    # a clip of length 0 adds exact zeros and is left out of the summary
    z = multi(g, o, [4000, 0, 4000, 4000])
    assert (_bits(z.sc_den)[:, 1] == 0).all()
    assert set(z.summary([4000, 0, 4000, 4000])) == set(s)


# ------------------------------------------------------------- the cepstra
@pytest.mark.parametrize('F', [1, 63, 64, 65, 200])
@pytest.mark.parametrize('C,K', [(80, 13), (5, 4), (128, 64), (3, 1)])
def test_cepstral_distance_against_the_restatement(hip_lib, C, K, F):
    from wavenet import spectral
    a, b = R.logmel_pair(1000 * C + F, 3, F, C)
    nf = np.array([F, (F + 1) // 2, 0])
    want, bound = R.mcd_sums(a, b, nf, K)
    got = spectral.cepstral_distance(a, b, nf, K)
    assert got.dtype == torch.float64 and got.shape == (3,)
    v = got.cpu().numpy()
    print('C %d K %d F %d: err %s bound %s' % (C, K, F, np.abs(v - want),
                                                bound))
    assert (np.abs(v - want) <= bound).all()
    assert _bits(got)[2] == 0                      # no frames: +0.0
    assert spectral.mcd_db(got, nf) == pytest.approx(
        R.mcd_db(a, b, nf, K), rel=1e-12)
    # the numpy form of the package, within the same bound
    assert (np.abs(spectral.cepstral_reference(a, b, nf, K) - want)
            <= bound).all()
    # equal tensors: exact zeros; no nframes: all frames
    assert (_bits(spectral.cepstral_distance(a, a.copy(), nf, K)) == 0).all()
    full = spectral.cepstral_distance(a, b, None, K)
    assert torch.equal(_bits(full), _bits(spectral.cepstral_distance(
        a, b, [F] * 3, K)))
    # a clip alone, at every position of a batch, and a NaN in a neighbour
    for clip in range(2):
        alone = _bits(spectral.cepstral_distance(a[clip], b[clip],
                                                 nf[clip:clip + 1], K))
        for shift in range(3):
            idx = np.roll(np.arange(3), shift)
            pos = int(np.where(idx == clip)[0][0])
            bad = a[idx].copy()
            bad[(pos + 1) % 3, 0, 0] = np.nan
            got = spectral.cepstral_distance(bad, b[idx], nf[idx], K)
            assert _bits(got)[pos] == alone[0], (clip, shift)
    bad = a.copy()
    bad[0, F - 1, C - 1] = np.nan
    assert np.isnan(spectral.cepstral_distance(bad, b, nf, K)[0].item())
