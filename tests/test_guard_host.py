"""tests/guard.py on CPU tensors: faults planted with plain torch ops are
reported with the operand, the band and the offset; a clean op passes.  And
the coverage rule: every wn_* entry of include/wavenet_hip.h that writes
through a pointer is a row of tests/test_gpu_guard_entries.py or carries a
written exemption there."""
import os
import re

import numpy as np
import pytest
import torch

import guard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _arena():
    a = guard.Arena('cpu')
    x = a.place('x', np.arange(35, dtype=np.float32).reshape(5, 7),
                torch.float32)
    y = a.place('y', (5, 7), torch.float32, ld=12, role='out')
    q = a.place('q', np.arange(10) % 16, torch.int32, fill=(15, 0))
    return a, x, y, q


def _flat(t, n, offset=0):
    """n words of t's storage from `offset` words after t's first element
    (plain torch: the view a kernel's pointer arithmetic amounts to)"""
    return torch.as_strided(t, (n,), (1,), t.storage_offset() + offset)


def test_layout_alignment_and_patterns():
    a, x, y, q = _arena()
    for name, skew in (('x', 0), ('y', 0), ('q', 0)):
        assert a.ptr(name) % 256 == skew
    s = a.place('skewed', (3,), torch.float32, skew_bytes=4)
    assert s.data_ptr() % 256 == 4
    d = a.place('d', (3,), torch.float64, role='out')
    assert d.data_ptr() % 256 == 0
    # bands: one 128-row tile at the leading dimension, at least 4096 words
    assert a.ops['x'].band == 4096 and a.ops['y'].band == 4096
    wide = a.place('wide', (2, 256), torch.float32, ld=260)
    assert a.ops['wide'].band == 128 * 260
    # the words either side of x and the gap columns of y hold the pattern
    assert int(_flat(x, 1, -1).view(torch.int32)) == guard.NAN32
    assert int(_flat(x, 1, 35).view(torch.int32)) == guard.NAN32
    assert int(_flat(y, 1, 7).view(torch.int32)) == guard.NAN32
    assert int(_flat(y, 1, 4 * 12 + 11).view(torch.int32)) == guard.NAN32
    assert int(_flat(d, 1, 3).view(torch.int64)) == guard.NAN64
    assert bool(torch.isnan(_flat(x, 1, 35))) and \
        guard.NAN32 != int(np.array([np.nan], np.float32).view(np.int32)[0])
    # integer bands hold a value that is valid where it would be read
    assert int(_flat(q, 1, 10)) == 15 and int(_flat(q, 1, -1)) == 15
    a.refill('B')
    assert int(_flat(q, 1, 10)) == 0
    assert float(_flat(x, 1, 35)) == 0.0 and float(_flat(x, 1, -1)) == 0.0
    # ('out' operands keep the NaN pattern: nothing may depend on them)
    assert int(_flat(y, 1, 7).view(torch.int32)) == guard.NAN32
    a.check()
    assert y.shape == (5, 7) and y.stride() == (12, 1)
    assert torch.equal(x, torch.arange(35.).reshape(5, 7))


def test_clean_op_passes():
    a, x, y, q = _arena()

    def run():
        y.copy_(x * 2 + q[:7].float())
    bits = guard.read_check(a, run)
    assert torch.equal(bits['y'].view(torch.float32),
                       x * 2 + q[:7].float())
    a.check()


def test_overrun_one_word_past_the_end():
    a, x, y, q = _arena()
    z = a.place('z', (35,), torch.float32, role='out')
    _flat(z, 36).copy_(torch.arange(36.))            # one word too many
    with pytest.raises(guard.GuardError) as e:
        a.check()
    assert (e.value.operand, e.value.band, e.value.offset, e.value.count) \
        == ('z', 'back', 1, 1)
    assert "'z'" in str(e.value) and 'back' in str(e.value)


def test_overrun_past_the_last_row_of_a_padded_operand():
    a, x, y, q = _arena()
    _flat(y, 3, 5 * 12 - 1).fill_(1.0)     # last gap word + 2 past the end
    with pytest.raises(guard.GuardError) as e:
        a.check()
    # (the last row's gap comes first in memory)
    assert (e.value.operand, e.value.band, e.value.offset, e.value.count) \
        == ('y', 'gap', (4, 11), 3)


def test_underrun_one_word_before_the_start():
    a, x, y, q = _arena()
    _flat(q, 1, -1).fill_(3)
    with pytest.raises(guard.GuardError) as e:
        a.check()
    assert (e.value.operand, e.value.band, e.value.offset, e.value.count) \
        == ('q', 'front', -1, 1)


def test_underrun_far_in_front():
    a, x, y, q = _arena()
    _flat(x, 2, -4096).fill_(0.0)
    with pytest.raises(guard.GuardError) as e:
        a.check()
    assert (e.value.operand, e.value.band, e.value.offset, e.value.count) \
        == ('x', 'front', -4096, 2)


def test_store_into_a_gap_column():
    a, x, y, q = _arena()
    _flat(y, 1, 2 * 12 + 7).fill_(0.5)               # row 2, column 7 of ld 12
    with pytest.raises(guard.GuardError) as e:
        a.check()
    assert (e.value.operand, e.value.band, e.value.offset, e.value.count) \
        == ('y', 'gap', (2, 7), 1)


def test_canonical_nan_store_over_the_band_is_seen():
    a, x, y, q = _arena()
    _flat(x, 2, 35).fill_(float('nan'))              # a NaN over a NaN band
    with pytest.raises(guard.GuardError) as e:
        a.check()
    assert (e.value.operand, e.value.band, e.value.offset, e.value.count) \
        == ('x', 'back', 1, 2)


def test_write_of_an_input_band_is_seen_in_both_variants():
    for variant in 'AB':
        a, x, y, q = _arena()
        a.refill(variant)
        _flat(q, 1, 10).fill_(7)
        with pytest.raises(guard.GuardError) as e:
            a.check()
        assert (e.value.operand, e.value.band, e.value.offset) == \
            ('q', 'back', 1)


def test_result_that_depends_on_a_band_word():
    a, x, y, q = _arena()

    def run():                     # row sums that run one word past x's end
        y.copy_(x)
        y[4, 6] = _flat(x, 2, 34).sum()
    with pytest.raises(guard.GuardError) as e:
        guard.read_check(a, run)
    assert (e.value.operand, e.value.band, e.value.offset, e.value.count) \
        == ('y', 'read', 34, 1)


def test_result_that_depends_on_an_index_band_word():
    a, x, y, q = _arena()

    def run():                     # a gather whose last index is q[10]
        idx = _flat(q, 7, 4).long()
        y.copy_(x[:, idx % 7])
    with pytest.raises(guard.GuardError) as e:
        guard.read_check(a, run)
    assert e.value.operand == 'y' and e.value.band == 'read'
    assert e.value.offset == 6 and e.value.count == 5


def test_read_check_restores_inout_operands_between_the_runs():
    a = guard.Arena('cpu')
    p = a.place('p', np.ones(9, np.float32), torch.float32, role='inout')
    g = a.place('g', np.full(9, 0.5, np.float32), torch.float32)

    def run():
        p.sub_(g)
    bits = guard.read_check(a, run)
    assert torch.equal(bits['p'].view(torch.float32), torch.full((9,), 0.5))
    a.reset()
    a.untouched()
    p[3] = 2.0
    with pytest.raises(guard.GuardError) as e:
        a.untouched()
    assert (e.value.operand, e.value.band, e.value.offset) == ('p', 'body', 3)


# ---- coverage of the C ABI ------------------------------------------------
def _entries_that_write():
    """name -> the non-const pointer parameters of every int / long wn_*
    declaration of the header (the stream handle is not an operand)."""
    src = open(os.path.join(ROOT, 'include', 'wavenet_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', ' ', src, flags=re.S)
    out = {}
    for m in re.finditer(r'\b(?:int|long)\s+(wn_\w+)\s*\(([^)]*)\)\s*;', src):
        params = [' '.join(p.split()) for p in m.group(2).split(',')]
        w = [p for p in params if '*' in p and not p.startswith('const ')
             and not re.search(r'\bstream$', p)]
        if w:
            out[m.group(1)] = w
    return out


def test_header_parse_sees_the_abi():
    w = _entries_that_write()
    assert len(w) > 100
    assert w['wn_fill'] == ['float* p']
    assert w['wn_xent_score'] == ['float* row_nll', 'double* clip_nll',
                                  'int32_t* clip_count',
                                  'int32_t* clip_correct', 'float* scratch']
    assert 'wn_xent_partials' not in w and 'wn_version' not in w


def test_every_writing_entry_is_guarded_or_exempt():
    import test_gpu_guard_entries as tge
    w = _entries_that_write()
    table = set(r.entry for r in tge.ROWS)
    exempt = tge.EXEMPT
    for name, reason in exempt.items():
        assert isinstance(reason, str) and len(reason.split()) >= 4, name
    assert not table & set(exempt), sorted(table & set(exempt))
    unknown = (table | set(exempt)) - set(w)
    assert not unknown, 'not entries that write: %s' % sorted(unknown)
    missing = sorted(set(w) - table - set(exempt))
    assert not missing, \
        'entries without a guard row or an exemption: %s' % missing

