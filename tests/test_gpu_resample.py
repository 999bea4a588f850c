"""wn_resample on the device: bit for bit Resampler.reference at every tile
edge, at clips shorter than the filter, on each of the kernel's paths (whole
table / phase rows / taps from memory, input staged or not), in ragged batches,
through padded strides and `out=`; a NaN's reach; and the float64 restatement
(tests/resample_ref.py) within the bound measured on the host."""
import numpy as np
import pytest
import torch

import resample_ref as R

pytestmark = pytest.mark.gpu

RATIOS = [(5, 8), (5, 12), (5, 4), (100, 441)]
_cache = {}


def _rs(up, down, half_width=10):
    from wavenet import resample
    key = (up, down, half_width)
    if key not in _cache:
        _cache[key] = resample.Resampler(down * 100, up * 100,
                                         half_width=half_width)
    return _cache[key]


def _signal(B, T, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(T)
    return (0.5 * np.sin(0.05 * t)[None, :] +
            0.2 * rng.standard_normal((B, T))).astype(np.float32)


def _n_for(rs, length):
    """The shortest clip with out_length(n) >= length: == length when
    downsampling; when upsampling, where out_length skips values, at most one
    more."""
    n = (length - 1) * rs.down // rs.up + 1
    assert rs.out_length(n) >= length > rs.out_length(n - 1)
    assert rs.out_length(n) == length or (rs.up > rs.down and
                                          rs.out_length(n) == length + 1)
    return n


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32)


def _same(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    g, w = _bits(got), _bits(want)
    bad = np.argwhere(g != w)
    assert not len(bad), (len(bad), bad[:4].tolist())


@pytest.mark.parametrize('half_width', [1, 10])
@pytest.mark.parametrize('up,down', RATIOS)
def test_tile_edges_and_short_clips(hip_lib, up, down, half_width):
    rs = _rs(up, down, half_width)
    tile = rs.tile()
    n = [_n_for(rs, L) for L in (1, tile - 1, tile, tile + 1, 2 * tile + 3)]
    # clips inside the filter's half length: every window clipped at both ends
    n += [1, 2, max(rs.Hh // up, 1), rs.Hh // up + 1]
    T = max(n)
    x = _signal(len(n), T, up + down)
    got = rs(x, n)
    _same(got, rs.reference(x, n))
    # ... and each clip alone, at its own T
    for b in (1, 3, 6, 8):
        _same(rs(x[b, :n[b]]), rs.reference(x[b, :n[b]]))


# (up, down, half_width, n): whole table with the input read from memory;
# the rows of the tile's phases; taps and input from memory (two tiles); taps
# from memory with the input staged
PATHS = [(1, 13, 10, 4000), (1000, 1001, 10, 300), (1, 1000, 10, 257500),
         (300, 301, 32, 520)]


@pytest.mark.parametrize('up,down,half_width,n', PATHS)
def test_every_kernel_path(hip_lib, up, down, half_width, n):
    rs = _rs(up, down, half_width)
    x = _signal(2, n, 5)
    lengths = [n, n // 2 + 1]
    _same(rs(x, lengths), rs.reference(x, lengths))


def test_ragged_batch_against_each_clip_alone(hip_lib):
    rs = _rs(5, 8)
    T = 1300
    n = [T, 0, 1, 777, 410]
    x = _signal(5, T, 11)
    poisoned = x.copy()
    for b in range(5):
        poisoned[b, n[b]:] = np.nan          # nothing behind n[b] is read
    got = rs(poisoned, n).cpu().numpy()
    _same(got, rs.reference(x, n))
    for b in range(5):
        no = rs.out_length(n[b])
        assert not got[b, no:].view(np.int32).any()      # exact +0
        if n[b]:
            _same(rs(x[b, :n[b]]), got[b, :no])
    # the same clips at other positions, in another B and at another T
    order = [3, 0, 4]
    wide = np.zeros((3, T + 500), np.float32)
    wide[:, :T] = x[order]
    again = rs(wide, [n[b] for b in order]).cpu().numpy()
    for i, b in enumerate(order):
        _same(again[i, :got.shape[1]], got[b])
        assert not again[i, got.shape[1]:].view(np.int32).any()


def test_padded_strides_and_out(hip_lib):
    rs = _rs(5, 8)
    B, T = 3, 1000
    To = rs.out_length(T)
    x = _signal(B, T, 2)
    n = [1000, 513, 90]
    want = rs.reference(x, n)
    big = torch.full((B, T + 3), float('nan'), device='cuda')
    big[:, :T] = torch.from_numpy(x)
    src = big[:, :T]
    assert src.stride(0) == T + 3
    _same(rs(src, n), want)
    hold = torch.full((B, To + 5), 7.0, device='cuda')
    out = hold[:, :To]
    back = rs(src, n, out=out)
    assert back is out
    _same(out, want)
    assert (hold[:, To:] == 7.0).all()
    with pytest.raises(ValueError):
        rs(src, n, out=torch.zeros((B, To + 1), device='cuda'))
    with pytest.raises(ValueError):          # out overlaps audio
        rs(big[:, :T], n, out=big.reshape(-1)[:B * To].reshape(B, To))
    # one clip, [T] in and [out_length(T)] out
    o1 = torch.empty(To, device='cuda')
    assert rs(x[0], out=o1) is o1
    _same(o1, want[0])


def test_equal_rates_copy(hip_lib):
    from wavenet import resample
    rs = resample.Resampler(8000, 8000)
    x = _signal(2, 700, 4)
    x[0, 5] = np.nan
    x[1, 9] = -0.0
    got = rs(x, [700, 300])
    _same(got, rs.reference(x, [700, 300]))
    assert np.array_equal(_bits(got)[0], x[0].view(np.int32))


@pytest.mark.parametrize('up,down,half_width', [(5, 8, 10), (5, 4, 10),
                                                (100, 441, 1)])
def test_a_nan_reaches_only_the_outputs_whose_taps_cover_it(hip_lib, up, down,
                                                            half_width):
    rs = _rs(up, down, half_width)
    n = _n_for(rs, rs.tile() + 40)
    j = _n_for(rs, rs.tile()) - 1            # its reach straddles a tile edge
    x = _signal(1, n, 9)[0]
    x[j] = np.nan
    got = rs(x).cpu().numpy()
    bad = np.nonzero(~np.isfinite(got))[0]
    want = R.reach(j, n, up, down, rs.Hh)
    assert len(want) and np.array_equal(bad, want)


@pytest.mark.parametrize('up,down', RATIOS + [(1000, 1001)])
def test_float64_restatement_within_the_measured_bound(hip_lib, up, down):
    rs = _rs(up, down)
    n = _n_for(rs, rs.tile() + 9)
    x = _signal(1, n, 21)[0]
    got = rs(x).cpu().numpy().astype(np.float64)
    tol, y64 = R.bound(x, up, down, rs.taps,
                       [rs.reference(x),
                        R.reversed_order32(x, up, down, rs.taps)])
    err = float(np.abs(got - y64).max())
    print('wn_resample %d/%d: error %.3e, bound %.3e, ratio %.3f'
          % (up, down, err, tol, err / tol))
    assert err <= tol
