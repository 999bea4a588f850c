"""Which branches of the persistent stack launches (csrc/wn_stack.hip) a
dilation list reaches: a host restatement of the tile arithmetic of the
forward kernels (`lo_row = t0 - d`, `first` / `last`, lanes 0 / 1) and of the
backward kernels' `flag_idx2` (`hif`, `first` / `last`), counted per
(dilation list, clip length T, tile height R) for one clip.

With power-of-two dilations a tap window is either tile-aligned (d >= R) or
reaches only into the tile before the wave's own (d < R), so lane 1's wait --
the tap that straddles TWO foreign tiles -- and a tap that starts inside a
later tile never run.  The lists DIL_A / DIL_B / DIL_C of tests/util.py are
what the GPU tests use to reach them; this file is the guard that keeps those
cases from becoming vacuous when somebody edits a list."""
import pytest

from util import DEFAULT, DIL_A, DIL_B, DIL_C, DIL_GEN, MID


def tile_classes(dilations, T, R):
    """Counts over the (layer, tile) pairs of ONE clip of T rows in tiles of R:

    fwd2   forward, layer l >= 1 (layer 0 waits on nothing): the tap rows
           t0-d .. t0-d+R-1 lie in two tiles and neither is the wave's own
           (lane 0 waits for `first`, lane 1 for `last`)
    bwd2   backward, layer l < L - 1: the rows t + dn (dn the dilation of the
           layer above) of the tile lie in two later tiles, neither its own
    part   forward, layer l >= 1, tile tt >= 1: the first d - t0 rows
           (0 < d - t0 < R) have no tap, the others read a foreign tile of
           the same clip -- with B > 1 the guard that keeps the tap out of
           the previous clip's rows
    hif    backward: 0 < hif < hi, the rows t + dn cut by the clip's end
           inside the tile
    """
    L = len(dilations)
    nt = -(-T // R)
    n = dict(fwd2=0, bwd2=0, part=0, hif=0)
    for l, d in enumerate(dilations):
        for tt in range(nt):
            t0 = tt * R
            hi = min(R, T - t0)
            lo_row = t0 - d
            if l > 0 and lo_row + R - 1 >= 0:
                first, last = max(lo_row, 0) // R, (lo_row + R - 1) // R
                if first != tt and last != first and last != tt:
                    n['fwd2'] += 1
                if tt >= 1 and 0 < d - t0 < R:
                    assert first == 0 != tt
                    n['part'] += 1
            if l + 1 < L:
                dn = dilations[l + 1]
                hif = min(hi, T - dn - t0)
                if hif > 0:
                    first, last = (t0 + dn) // R, (t0 + dn + hif - 1) // R
                    if first != tt and last != first and last != tt:
                        n['bwd2'] += 1
                    if hif < hi:
                        n['hif'] += 1
    return n


def _pow2(d):
    return d & (d - 1) == 0


# (list, T, R) -> fwd2, bwd2, part, hif: the shapes of tests/test_gpu_stack.py,
# test_gpu_model.py and test_gpu_local_condition.py
COUNTS = [
    ('A', DIL_A, 333, 32, (34, 34, 4, 9)),
    ('B', DIL_B, 150, 16, (21, 21, 3, 6)),
    ('C', DIL_C, 1100, 32, (164, 164, 7, 11)),
]


@pytest.mark.parametrize('name,dil,T,R,want', COUNTS,
                         ids=[c[0] for c in COUNTS])
def test_counts_of_the_named_lists(name, dil, T, R, want):
    n = tile_classes(dil, T, R)
    assert (n['fwd2'], n['bwd2'], n['part'], n['hif']) == want, n


REACH = [
    # (list, T, tile heights, classes that must occur)
    ('A_T333', DIL_A, 333, (32, 16), ('fwd2', 'bwd2', 'part', 'hif')),
    ('A_T301', DIL_A, 301, (32, 16), ('fwd2', 'bwd2', 'part', 'hif')),
    ('B_T150', DIL_B, 150, (16, 32), ('fwd2', 'bwd2', 'part', 'hif')),
    ('C_T1100', DIL_C, 1100, (32, 16), ('fwd2', 'bwd2', 'part', 'hif')),
    # two tiles per clip: no tap can straddle two FOREIGN tiles; the partial
    # tap at tile 1 and the cut by the clip's end remain
    ('A_T47', DIL_A, 47, (32,), ('part', 'hif')),
    ('A_T47_16', DIL_A, 47, (16,), ('fwd2', 'bwd2', 'part', 'hif')),
    ('tiny_T131', [3, 5, 6, 7, 9, 33, 47], 131, (16, 32),
     ('fwd2', 'bwd2', 'part', 'hif')),
]


@pytest.mark.parametrize('name,dil,T,rows,kinds', REACH,
                         ids=[c[0] for c in REACH])
def test_every_class_is_reached(name, dil, T, rows, kinds):
    for R in rows:
        n = tile_classes(dil, T, R)
        for k in kinds:
            assert n[k] >= 1, (name, R, k, n)


def test_short_clips_and_aligned_dilations():
    # T = 47: four layers of DIL_A have no tap inside the clip at all, and
    # tile 1 is partial
    assert sum(d >= 47 for d in DIL_A) == 4 and 47 % 32 and 47 % 16
    # a dilation that is a whole number of tiles without being a power of two
    for dil in (DIL_A, DIL_C):
        assert any(d % 32 == 0 and not _pow2(d) for d in dil)
    # one off a tile edge, both sides
    assert {31, 33, 63} <= set(DIL_A) and 513 in DIL_C
    assert sum(DIL_C) + 1 == 2605          # receptive field of DIL_C
    assert 2605 > 2 * 1100                 # (taps far behind the clip's start)


def test_generator_list_and_chunk_boundaries():
    """tests/test_gpu_dilations.py: no dilation a power of two, receptive
    field 114, and the chunk boundaries (101, 101 + 83) and admission steps
    (37, 101) are multiples of no dilation, so every ring is re-entered with
    its cursor inside the ring."""
    assert sum(DIL_GEN) + 1 == 114
    assert not any(_pow2(d) for d in DIL_GEN)
    for n in (101, 184, 37):
        assert all(n % d for d in DIL_GEN), n
    assert 2 < min(DIL_GEN) and min(DIL_GEN) < 40 < max(DIL_GEN) and 150 > 114
    assert 260 >= 5 * max(DIL_GEN)


@pytest.mark.parametrize('R', [16, 32])
@pytest.mark.parametrize('name,dil,T', [
    ('DEFAULT', DEFAULT['dilations'], 5211),
    ('DEFAULT_16000', DEFAULT['dilations'], 16000),
    ('MID', MID['dilations'], 300),
    ('pow2_T333', [1, 2, 4, 8, 16, 32, 64, 128], 333)])
def test_power_of_two_lists_reach_none(name, dil, T, R):
    """the gap: what every GPU case ran before the lists above"""
    n = tile_classes(dil, T, R)
    assert (n['fwd2'], n['bwd2'], n['part']) == (0, 0, 0), n
