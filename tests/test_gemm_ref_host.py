"""CPU side of the exact-operand GEMM tests: the premise of
tests/test_gpu_gemm_exact.py is proved here instead of trusted -- for every
family and shape the GPU file runs, float32 sums in three orders equal the
float64 result bit for bit -- and the argument checks of wn_gemm_nn that keep
the epilogue's 32-bit offsets in range are exercised without a device (they
return before any launch, as in tests/test_abi.py)."""
import ctypes

import numpy as np
import pytest

import gemm_ref as R

SEED = 20


def _same_bits(a, b):
    return np.array_equal(R.bits(a), R.bits(b))


def _check_orders(terms, ref64, post=lambda x: x):
    want = R.exact32(ref64)
    for got in R.sum_orders(terms):
        assert _same_bits(post(got), want)


@pytest.mark.parametrize('name,M,N,K', R.NN_CASES, ids=[c[0] for c in R.NN_CASES])
def test_family_a_nn_is_exact_in_any_order(name, M, N, K):
    o = R.family_a_nn(M, N, K, SEED)
    c64, pre64 = R.nn_ref(o['A'], o['W'], o['bias'], 1, o['mask'], o['add'])
    terms = R.nn_terms(o['A'], o['W'])
    _check_orders(terms, pre64, lambda s: s + o['bias'])
    _check_orders(terms, c64, lambda s: R.nn_epilogue(s + o['bias'], 1, o['mask'], o['add']).astype(np.float32))
    # without an epilogue the row exponents use all of +-20
    o = R.family_a_nn(M, N, K, SEED, epilogue=False)
    _check_orders(R.nn_terms(o['A'], o['W']), R.nn_ref(o['A'], o['W'])[1])
    assert np.abs(np.log2(np.abs(o['A'][o['A'] != 0]))).max() <= 23


def test_family_a_epilogues_are_exact():
    M, N, K = R.EPILOGUE_SHAPE
    o = R.family_a_nn(M, N, K, SEED)
    # every mask value class is present, and both signs of the pre-activation
    for v in R.MASK_VALUES:
        assert (R.bits(o['mask']) == R.bits(v)).any()
    terms = R.nn_terms(o['A'], o['W'])
    sums = R.sum_orders(terms)
    for e in range(32):
        bias = o['bias'] if e & 16 else None
        relu, mask = e & 1, o['mask'] if e & 2 else None
        add = o['add'] if e & 4 else None
        c64, pre64 = R.nn_ref(o['A'], o['W'], bias, relu, mask, add)
        assert (pre64 < 0).any() and (pre64 > 0).any()
        want_c, want_p = R.exact32(c64), R.exact32(pre64)
        for s in sums:
            pre = s if bias is None else s + bias
            assert _same_bits(pre, want_p)
            assert _same_bits(R.nn_epilogue(pre, relu, mask, add).astype(np.float32), want_c)


@pytest.mark.parametrize('name,M,P,X', R.PLANE_CASES, ids=[c[0] for c in R.PLANE_CASES])
def test_family_a_plane_shapes_are_exact(name, M, P, X):
    for MM, NN, KK in ((M, X, 32 * P), (M, 32 * P, X)):
        if KK % 4:
            continue
        o = R.family_a_nn(MM, NN, KK, SEED)
        c64, pre64 = R.nn_ref(o['A'], o['W'], o['bias'], 1, o['mask'], o['add'])
        terms = R.nn_terms(o['A'], o['W'])
        _check_orders(terms, c64, lambda s: R.nn_epilogue(s + o['bias'], 1, o['mask'], o['add']).astype(np.float32))


@pytest.mark.parametrize('name,rows,Mw,Nw,splits,cs', R.TN_CASES, ids=[c[0] for c in R.TN_CASES])
def test_family_a_tn_is_exact_in_any_order(name, rows, Mw, Nw, splits, cs):
    o = R.family_a_tn(rows, Mw, Nw, SEED)
    dw64, cs64 = R.tn_ref(o['A'], o['G'])
    # (the contraction runs over rows: A^T is the NN problem's A; the widest
    # shapes are checked on a corner of the output, every row kept)
    m, n = min(Mw, 48), min(Nw, 40)
    _check_orders(R.nn_terms(o['A'].T[:m], o['G'][:, :n]), dw64[:m, :n])
    _check_orders(o['G'], cs64)
    # slab sums: any split of the rows, summed slab by slab
    rps = -(-rows // splits)
    rps = -(-rps // 96) * 96
    slabs = np.stack([(o['A'][s * rps:(s + 1) * rps].astype(np.float64).T @
                       o['G'][s * rps:(s + 1) * rps].astype(np.float64)).astype(np.float32)
                      for s in range(splits)])
    _check_orders(slabs, dw64)


@pytest.mark.parametrize('name,B,T,Q,Nw,shift,splits', R.ONEHOT_CASES, ids=[c[0] for c in R.ONEHOT_CASES])
def test_one_hot_operand(name, B, T, Q, Nw, shift, splits):
    rng = np.random.default_rng(SEED)
    codes = rng.integers(0, Q, B * T)
    A = R.one_hot(codes, shift, T, Q)
    # by the definition: clip b, time t >= shift selects codes[b][t - shift]
    want = np.zeros((B * T, Q), np.float32)
    for b in range(B):
        for t in range(shift, T):
            want[b * T + t, codes[b * T + t - shift]] = 1
    assert np.array_equal(A, want)
    assert A[np.arange(B * T) % T < shift].sum() == 0
    G = R.family_a_tn(B * T, 4, Nw, SEED)['G']
    _check_orders(R.nn_terms(A.T[:32], G), R.tn_ref(A, G)[0][:32])


def test_split3_restates_the_kernel():
    rng = np.random.default_rng(SEED)
    x = np.concatenate([rng.standard_normal(4096).astype(np.float32),
                        R.family_b_nn('b2', 8, 8, 16, SEED)['A'].ravel(),
                        np.array([0.0, 1.0, -1.0, 257.0, 65793.0, 2.0 ** -100], np.float32)])
    hi, mi, lo = R.split3(x)
    # exact, and every piece has at most 8 significant bits (a bf16 number)
    assert np.array_equal(hi.astype(np.float64) + mi.astype(np.float64) + lo.astype(np.float64),
                          x.astype(np.float64))
    for p in (hi, mi, lo):
        assert not (R.bits(p) & np.uint32(0xffff)).any()
    assert np.all(np.abs(mi) <= np.abs(hi) * 2.0 ** -7) and np.all(np.abs(lo) <= np.abs(mi) * 2.0 ** -7)
    assert R.split3(np.float32(65793.0))[1] == 256 and R.split3(np.float32(65793.0))[2] == 1


_B_NN = [(k,) + c for k in R.B_KINDS for c in R.NN_B_CASES]


@pytest.mark.parametrize('kind,name,M,N,K', _B_NN, ids=['%s-%s' % c[:2] for c in _B_NN])
def test_family_b_is_exact_and_sees_its_products(kind, name, M, N, K):
    o = R.family_b_nn(kind, M, N, K, SEED)
    full = o['A'].astype(np.float64) @ o['W'].astype(np.float64)
    for nprod in (3, 6, 9):
        want = R.split_matmul(o['A'], o['W'], nprod)
        # every single piece product, in any order, in float32
        m, n = min(M, 40), min(N, 36)
        _check_orders(R.split_terms(o['A'][:m], o['W'][:, :n], nprod), want[:m, :n])
        R.exact32(want)
        for ik in R.PRODUCT_SETS[nprod]:
            changed = not np.array_equal(R.split_matmul(o['A'], o['W'], nprod, drop=ik), want)
            assert changed == (ik in R.B_SEES[kind]), (kind, nprod, ik)
        if nprod >= 6:
            assert np.array_equal(want, full)
    if kind == 'b2':
        # x3 returns A's elements truncated to their upper two pieces
        hi, mi, lo = R.split3(o['A'])
        assert (lo != 0).all()
        k = np.abs(o['W']).argmax(0)
        want3 = (hi + mi)[:, k].astype(np.float64) * o['W'][k, np.arange(N)].astype(np.float64)
        assert np.array_equal(R.split_matmul(o['A'], o['W'], 3), want3)
        assert not np.array_equal(want3, full)


def test_every_visible_product_is_seen_by_some_case():
    """Each product of an nprod's set that can be exact at all (i + k <= 4,
    gemm_ref's docstring) changes the expected result of at least one family
    (b) kind; the three x9 adds span at least 25 bits and cannot."""
    seen = set(p for k in R.B_KINDS for p in R.B_SEES[k])
    assert seen == set(R.VISIBLE)
    for nprod in (3, 6, 9):
        for i, k in R.PRODUCT_SETS[nprod]:
            assert ((i, k) in seen) == (i + k <= 2)
    # the smallest value with a nonzero piece i spans 8 i + 1 bits
    for i, v in ((1, 257.0), (2, 65793.0)):
        assert R.split3(np.float32(v))[i] != 0 and R.split3(np.float32(v - 1))[i] == 0
    assert 8 * (1 + 2) + 1 > 24


@pytest.mark.parametrize('name,rows,Mw,Nw,splits', R.TN_SPLIT_CASES, ids=[c[0] for c in R.TN_SPLIT_CASES])
def test_family_b_tn_shapes_are_exact(name, rows, Mw, Nw, splits):
    for kind in R.B_KINDS:
        o = R.family_b_tn(kind, rows, Mw, Nw, SEED)
        for nprod in (3, 6, 9):
            want = R.split_matmul(np.ascontiguousarray(o['A'].T), o['G'], nprod)
            R.exact32(want)
            m, n = min(Mw, 24), min(Nw, 24)
            _check_orders(R.split_terms(np.ascontiguousarray(o['A'].T[:m]), o['G'][:, :n], nprod),
                          want[:m, :n])


def test_yardstick_matches_its_definition():
    rng = np.random.default_rng(SEED)
    A = rng.standard_normal((37, 64)).astype(np.float32)
    W = rng.standard_normal((64, 20)).astype(np.float32)
    b = rng.standard_normal(20).astype(np.float32)
    ref, e32 = R.yardstick(A, W, b)
    acc = np.zeros((37, 20), np.float32)
    for k in range(64):
        acc = acc + np.outer(A[:, k], W[k])
    assert np.array_equal(acc + b, R.f32_forward(A, W, b))
    assert e32 == np.abs((acc + b).astype(np.float64) - ref).max() and 0 < e32 < 1e-4
    # the dropped terms: x9 none, x6 ~2^-24, x3 ~2^-16 of |a||w| per product
    d = [np.abs(R.split_matmul(A, W, n) - A.astype(np.float64) @ W.astype(np.float64)).max() for n in (3, 6, 9)]
    assert d[2] < 1e-12 < d[1] < 1e-5 < d[0] < 1e-2   # (x9: float64 rounding of nine matmuls)
    assert R.yardstick(A, W, b, 3)[1] == e32 + d[0] and R.yardstick(A, W, b, 9)[1] == e32


def test_layout_indices():
    assert R.dense_index(3, 4, 10).tolist() == [[0, 1, 2, 3], [10, 11, 12, 13], [20, 21, 22, 23]]
    p = R.plane_index(2, 64, 100)
    assert p[0, 0] == 0 and p[1, 0] == 32 and p[0, 31] == 31 and p[0, 32] == 100 and p[1, 63] == 163


# ---- argument checks of wn_gemm_nn (no launch) ------------------------------
LD_MAX = 17318412                    # (31 ld + 64) * 4 <= 2^31 - 1, ld % 4 == 0
CPS_MAX = 2 ** 29 - 1028             # c_plane_stride * 4 + 4096 <= 2^31 - 1


def test_epilogue_offsets_are_refused_beyond_32_bits(hip_lib):
    """gemm_epilogue / gemm_epilogue_wide reach the rows of a 32-row half
    through 32-bit byte offsets of a buffer resource that ends at 2^31 - 1: the
    last access lies (31 ld + 60) * 4 bytes in.  The first leading dimension
    past that is WN_ERR_UNSUPPORTED.  The last one inside passes every check:
    shown with a misaligned W, whose WN_ERR_MISALIGNED is the last check before
    the launch."""
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    assert (31 * LD_MAX + 64) * 4 <= 2 ** 31 - 1 < (31 * (LD_MAX + 4) + 64) * 4
    assert CPS_MAX * 4 + 4096 <= 2 ** 31 - 1 < (CPS_MAX + 4) * 4 + 4096
    UNSUPPORTED, MISALIGNED = -2, -3

    def both(**kw):
        """(code with the arguments as given, code with W misaligned)"""
        p = dict(lda=16, ldw=64, mask=None, ld_mask=0, add=None, ld_add=0, ldc=64, c_planes=0,
                 cps=0, cpre=None, M=32, N=64, K=16)
        p.update(kw)
        return hip_lib.wn_gemm_nn(a, p['lda'], 0, 0, a + 4, p['ldw'], None, p['mask'], p['ld_mask'],
                                  p['add'], p['ld_add'], a, p['ldc'], p['c_planes'], p['cps'],
                                  p['cpre'], p['M'], p['N'], p['K'], 0, None)

    assert both() == MISALIGNED                      # the probe itself: past every check
    for key, extra in (('ldc', {}), ('ld_mask', dict(mask=a)), ('ld_add', dict(add=a)),
                       ('ldc', dict(c_planes=2, cps=4096, cpre=a))):
        assert both(**{key: LD_MAX}, **extra) == MISALIGNED, key
        assert both(**{key: LD_MAX + 4}, **extra) == UNSUPPORTED, key
        assert both(**{key: -4}, **extra) == UNSUPPORTED, key
        assert both(**{key: 2 ** 40}, **extra) == UNSUPPORTED, key
    # leading dimensions of operands that are not passed are not looked at
    assert both(ld_mask=LD_MAX + 4, ld_add=LD_MAX + 4) == MISALIGNED
    assert both(ldc=LD_MAX + 4, c_planes=2, cps=4096) == MISALIGNED     # plane C without Cpre
    # plane-mode C: the neighbour plane + 31 rows of 128 B
    assert both(c_planes=2, cps=CPS_MAX, ldc=0) == MISALIGNED
    assert both(c_planes=2, cps=CPS_MAX + 4, ldc=0) == UNSUPPORTED
    assert both(c_planes=2, cps=2 ** 29, ldc=0) == UNSUPPORTED          # c_plane_stride * 4 >= 2^31
    assert both(c_planes=2, cps=2 ** 29 - 4, ldc=0) == UNSUPPORTED
    assert both(c_planes=2, cps=-32, ldc=0) == UNSUPPORTED
    # the split entry shares the checks
    scratch = a
    for ld, want in ((LD_MAX, MISALIGNED), (LD_MAX + 4, UNSUPPORTED)):
        assert hip_lib.wn_gemm_nn_split(a, 16, 0, 0, a + 4, 64, None, None, 0, None, 0, a, ld, 0, 0,
                                        None, 32, 64, 16, 0, scratch, 6, None) == want
