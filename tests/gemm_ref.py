"""Operands and float64 references for the GEMM entry points (wn_gemm_nn,
wn_gemm_nn_split, wn_gemm_tn, wn_gemm_tn_split + the slab reductions).  numpy
only: tests/test_gemm_ref_host.py proves the statements made here on the CPU,
tests/test_gpu_gemm_exact.py holds the kernels against them.

Exact operands.  Every product and every partial sum of these operands, in any
order, is a float32 number, so a correct kernel equals the float64 result bit
for bit whatever its tiling, K split or slab count.

 (a) small integers: A, W / G, bias and addend are integers of magnitude <= 8;
     row i of A carries a factor 2^r_i and column j of W a factor 2^c_j (for
     the TN contraction over rows: column m of A and column n of G).  Element
     (i, j) of A W is then 2^(r_i + c_j) times an integer below K * 64 < 2^24.
     The addend is in the same scale, 2^(r_i + c_j) times an integer.  The bias
     has no row: it is 2^c_j times an integer, and 2^r_i S + b stays within 24
     bits only while 64 K 2^r_i < 2^23, so with an epilogue the row exponents
     are drawn from [-20, 23 - ceil(log2(64 K))] instead of [-20, 20].
 (b) pieces of the split-bf16 kernels, which cut a float by truncation into
     8 + 8 + 8 significant bits (split3) and add up 3, 6 or 9 of the nine piece
     products.  Piece i of one operand is nonzero only for a value that spans
     8 (i - 1) + 1 bits, so the product of pieces i and k spans at least
     8 (i + k - 2) + 1 bits: the six products of the x6 set (i + k <= 4) can be
     exact float32 numbers, the three x9 adds (i + k >= 5, at least 25 bits)
     cannot, and no exact case can see them.
     (b1) 16-bit integers against {-1, 0, 1} 2^f, K <= 128: pieces (1,1), (2,1)
     (b2) 24-bit integers against one power of two per column: + (3,1); the
          x3 set returns them truncated to their upper two pieces
     (b3) (b2) mirrored: one power of two per row of A, 24-bit W: (1,2), (1,3)
     (b4) odd 9-bit integers on both sides, K <= 128: + (2,2)
"""
import numpy as np

F32, F64, U32 = np.float32, np.float64, np.uint32

# pieces (of the first operand, of the second), 0 = high; the kernels' sets
PRODUCT_SETS = {
    3: [(0, 0), (0, 1), (1, 0)],
    6: [(0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0)],
    9: [(0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0), (2, 2), (1, 2), (2, 1)],
}
# the products an exact case can see (see above)
VISIBLE = PRODUCT_SETS[6]


def bits(x):
    return np.ascontiguousarray(x, F32).view(U32)


def exact32(ref64):
    """float64 reference -> float32, asserting nothing is lost; zeros are +0
    (the kernels' accumulators start at +0)."""
    ref64 = np.asarray(ref64, F64) + 0.0
    r32 = ref64.astype(F32)
    assert np.array_equal(r32.astype(F64), ref64), 'reference is not exact in float32'
    return r32


def _ints(rng, shape, mag=8):
    return rng.integers(-mag, mag + 1, shape).astype(F64)


def _pow2(e):
    return np.ldexp(1.0, np.asarray(e, np.int64))


def row_exp_max(K, epilogue):
    return min(20, 23 - int(np.ceil(np.log2(64 * K)))) if epilogue else 20


# mask values: the multiplier is (mask > 0)
MASK_VALUES = np.array([0.0, -0.0, -1e-45, 1e-45, -1.1754944e-38, 1.1754944e-38,
                        -1.0, 1.0, -3.5, 2.0 ** -20, -2.0 ** 20, 7.0], F32)


def family_a_nn(M, N, K, seed, epilogue=True):
    """dict(A [M][K], W [K][N], bias [N], mask [M][N], add [M][N]) float32."""
    assert K * 64 < 2 ** 24
    rng = np.random.default_rng([seed, M, N, K])
    r = rng.integers(-20, row_exp_max(K, epilogue) + 1, M)
    c = rng.integers(-20, 21, N)
    A = _ints(rng, (M, K)) * _pow2(r)[:, None]
    W = _ints(rng, (K, N)) * _pow2(c)[None, :]
    bias = _ints(rng, N) * _pow2(c)
    add = _ints(rng, (M, N)) * _pow2(r[:, None] + c[None, :])
    mask = MASK_VALUES[rng.integers(0, len(MASK_VALUES), (M, N))]
    f = lambda x: x.astype(F32)
    return dict(A=f(A), W=f(W), bias=f(bias), mask=mask, add=f(add))


def nn_epilogue(pre, relu, mask, add):
    x = np.maximum(pre, 0.0) if relu else pre
    if mask is not None:
        x = np.where(mask > 0, x, 0.0)
    if add is not None:
        x = x + add
    return x + 0.0


def nn_ref(A, W, bias=None, relu=0, mask=None, add=None):
    """(C, Cpre) in float64: C = epi(A W), Cpre = A W + bias."""
    pre = A.astype(F64) @ W.astype(F64)
    if bias is not None:
        pre = pre + bias.astype(F64)
    pre = pre + 0.0
    return nn_epilogue(pre, relu, mask, None if add is None else add.astype(F64)), pre


def family_a_tn(rows, Mw, Nw, seed):
    """dict(A [rows][Mw], G [rows][Nw]) float32 for dW = A^T G."""
    assert rows * 64 < 2 ** 24
    rng = np.random.default_rng([seed, rows, Mw, Nw])
    A = _ints(rng, (rows, Mw)) * _pow2(rng.integers(-20, 21, Mw))[None, :]
    G = _ints(rng, (rows, Nw)) * _pow2(rng.integers(-20, 21, Nw))[None, :]
    return dict(A=A.astype(F32), G=G.astype(F32))


def tn_ref(A, G):
    """(dW [Mw][Nw], column sums of G [Nw]) in float64."""
    return A.astype(F64).T @ G.astype(F64) + 0.0, G.astype(F64).sum(0) + 0.0


def one_hot(codes, shift, T, Q):
    """The A operand wn_gemm_tn generates from codes: row b T + t holds the
    one-hot of codes[b T + t - shift] for t >= shift, zeros before."""
    codes = np.asarray(codes).reshape(-1)
    rows = codes.size
    A = np.zeros((rows, Q), F32)
    t = np.arange(rows) % T
    ok = t >= shift
    r = np.nonzero(ok)[0]
    c = codes[r - shift]
    keep = (c >= 0) & (c < Q)
    A[r[keep], c[keep]] = 1.0
    return A


# ---- split-bf16 arithmetic ------------------------------------------------
def split3(x):
    """The kernels' split3: high, middle, low piece (float32 arrays)."""
    x = np.ascontiguousarray(x, F32)
    top = U32(0xffff0000)
    hi = (x.view(U32) & top).view(F32)
    r = x - hi
    mi = (r.view(U32) & top).view(F32)
    lo = ((r - mi).view(U32) & top).view(F32)      # (packed as bf16)
    return hi, mi, lo


def split_matmul(A, W, nprod, drop=None):
    """A W as the split kernels add it up, pieces in float64 (exact piece
    products, no accumulation error); drop: one product left out."""
    a, w = split3(A), split3(W)
    out = np.zeros((A.shape[0], W.shape[1]), F64)
    for ik in PRODUCT_SETS[nprod]:
        if ik != drop:
            out += a[ik[0]].astype(F64) @ w[ik[1]].astype(F64)
    return out + 0.0


def split_terms(A, W, nprod):
    """Every single piece product as a float32 array [terms][M][N]."""
    a, w = split3(A), split3(W)
    return np.concatenate([a[i].T[:, :, None] * w[k][:, None, :]
                           for i, k in PRODUCT_SETS[nprod]], 0)


def _int24(rng, shape):
    v = rng.integers(0, 2 ** 24, shape) | (2 ** 23 + 2 ** 15 + 1)   # three nonzero pieces
    return (v * rng.choice([-1, 1], shape)).astype(F64)


def _one_per_col(rng, K, N):
    W = np.zeros((K, N), F64)
    W[rng.integers(0, K, N), np.arange(N)] = rng.choice([-1, 1], N) * _pow2(rng.integers(-20, 21, N))
    return W


def family_b_nn(kind, M, N, K, seed):
    """dict(A [M][K], W [K][N]) float32 of family (b1) .. (b4)."""
    assert K <= 128
    rng = np.random.default_rng([seed, M, N, K, int(kind[1])])
    if kind == 'b1':
        A = rng.integers(-2 ** 16 + 1, 2 ** 16, (M, K)).astype(F64)
        W = _ints(rng, (K, N), 1) * _pow2(rng.integers(-20, 21, N))[None, :]
    elif kind == 'b2':
        A, W = _int24(rng, (M, K)), _one_per_col(rng, K, N)
    elif kind == 'b3':
        A, W = _one_per_col(rng, K, M).T.copy(), _int24(rng, (K, N))
    elif kind == 'b4':
        top = int(np.sqrt(2 ** 24 / K))            # K a^2 < 2^24
        assert top >= 259
        odd = lambda s: (2 * rng.integers(128, (top - 1) // 2 + 1, s) + 1) * rng.choice([-1, 1], s)
        A, W = odd((M, K)).astype(F64), odd((K, N)).astype(F64)
    else:
        raise ValueError(kind)
    return dict(A=A.astype(F32), W=W.astype(F32))


B_KINDS = ('b1', 'b2', 'b3', 'b4')
# the products each kind exposes (removing one changes the expected result)
B_SEES = {'b1': [(0, 0), (1, 0)], 'b2': [(0, 0), (1, 0), (2, 0)],
          'b3': [(0, 0), (0, 1), (0, 2)], 'b4': [(0, 0), (0, 1), (1, 0), (1, 1)]}


def family_b_tn(kind, rows, Mw, Nw, seed):
    """dict(A [rows][Mw], G [rows][Nw]): dW = A^T G is family (b)'s A W."""
    o = family_b_nn(kind, Mw, Nw, rows, seed)
    return dict(A=np.ascontiguousarray(o['A'].T), G=o['W'])


# ---- float32 evaluation orders (the CPU proof of exactness) ---------------
def sum_orders(terms):
    """Float32 sums of terms [T][...] in three orders: forward, reversed,
    pairwise (adjacent pairs, level by level)."""
    terms = np.ascontiguousarray(terms, F32)
    fwd = np.zeros(terms.shape[1:], F32)
    for t in terms:
        fwd = fwd + t
    rev = np.zeros(terms.shape[1:], F32)
    for t in terms[::-1]:
        rev = rev + t
    lvl = terms
    while lvl.shape[0] > 1:
        if lvl.shape[0] & 1:
            lvl = np.concatenate([lvl, np.zeros((1,) + lvl.shape[1:], F32)], 0)
        lvl = lvl[0::2] + lvl[1::2]
    return fwd, rev, lvl[0]


def nn_terms(A, W):
    """The K products of every output element, float32 [K][M][N]."""
    return A.astype(F32).T[:, :, None] * W.astype(F32)[:, None, :]


# ---- layouts ----------------------------------------------------------------
def dense_index(M, X, ld):
    """flat positions [M][X] of a dense operand with leading dimension ld"""
    return np.arange(M, dtype=np.int64)[:, None] * ld + np.arange(X, dtype=np.int64)[None, :]


def plane_index(M, X, stride):
    """flat positions [M][X] of X / 32 planes of [M][32], `stride` apart"""
    j = np.arange(X, dtype=np.int64)[None, :]
    return (j >> 5) * stride + np.arange(M, dtype=np.int64)[:, None] * 32 + (j & 31)


# ---- the measured yardstick (normal data) -----------------------------------
def f32_forward(A, W, bias=None):
    """Plain float32 restatement: k = 0, 1, ... one multiply and one add each,
    then the bias (A [M][K], W [K][N])."""
    A, W = A.astype(F32), W.astype(F32)
    acc = np.zeros((A.shape[0], W.shape[1]), F32)
    for k in range(A.shape[1]):
        acc += A[:, k:k + 1] * W[k:k + 1, :]
    return acc if bias is None else acc + bias.astype(F32)


def yardstick(A, W, bias=None, nprod=0):
    """(ref64, e32): e32 = max error of f32_forward against float64, plus -- for
    the x3 / x6 product sets -- the largest dropped-term error of split_matmul."""
    ref = A.astype(F64) @ W.astype(F64)
    drop = np.abs(split_matmul(A, W, nprod) - ref).max() if nprod in (3, 6) else 0.0
    if bias is not None:
        ref = ref + bias.astype(F64)
    return ref, float(np.abs(f32_forward(A, W, bias) - ref).max() + drop)


# ---- the shapes (shared by the host proof and the GPU tests) ----------------
# The id names the kernel the host's dispatch picks (wn_gemm.hip,
# gemm_nn_launch / wn_gemm_tn): K % 16 == 0 -> gemm_nn3 (LDS-DMA, 16-deep
# chunks), else gemm_nn<2> (register staging, 32-deep chunks); the split entry
# takes K % 16 == 0 only (32-deep chunks: K = 16, 48 leave the last half empty).
NN_CASES = [
    ('reg-1chunk-M1', 1, 4, 4),
    ('dma-1chunk', 127, 64, 16),
    ('reg-ragged-k', 128, 68, 20),
    ('dma-2chunks', 129, 128, 32),
    ('dma-3chunks-2coltiles', 257, 132, 48),
    ('reg-3chunks-deadwaves', 129, 192, 68),
    ('dma-deadwaves', 257, 192, 32),
    ('dma-long', 127, 132, 512),
    ('dma-M1', 1, 68, 16),
]
# (b): K <= 128, K % 16 == 0
NN_B_CASES = [('1chunk', 129, 68, 16), ('halfchunk', 127, 132, 48), ('4chunks', 257, 192, 128)]
# planes: (id, M, P, other width)
PLANE_CASES = [('P1', 129, 1, 68), ('P2', 257, 2, 132), ('P5', 127, 5, 64)]
# all sixteen epilogues x bias at one edge shape
EPILOGUE_SHAPE = (129, 132, 48)

# TN: Mw % 128 or 160 == 0 and Nw % 128 == 0 -> the workgroup-tile kernels
# (gemm_tn3, LDS-DMA, while a split's rows fit 32-bit offsets), else the
# LDS-free wave-tile kernel gemm_tn<MF, NF>.  (id, rows, Mw, Nw, splits, colsum)
TN_CASES = [
    ('dma41-1chunk', 16, 128, 128, 1, 1),
    ('dma51', 96, 160, 128, 3, 1),
    ('dma42-raggedrows-spread', 100, 128, 256, 3, 2),
    ('dma51x2-emptysplits', 1603, 160, 256, 40, 1),
    ('dma41-nocolsum', 1603, 128, 128, 3, 0),
    ('dma41-moresplitsthanchunks-spread', 96, 128, 128, 40, 2),
    ('wave11', 16, 32, 32, 1, 1),
    ('wave-ragged', 100, 100, 36, 3, 1),
    ('wave12-fast-emptysplits', 1603, 96, 64, 40, 1),
    ('wave21-nocolsum', 96, 64, 96, 1, 0),
    ('wave-ragged-long', 1603, 36, 100, 3, 1),
]
# wn_gemm_tn_split: rows % 16 == 0; (id, rows, Mw, Nw, splits)
TN_SPLIT_CASES = [('1chunk', 16, 128, 128, 1), ('ragged-tiles', 96, 132, 68, 3),
                  ('emptysplits', 96, 160, 128, 40), ('8chunks', 128, 36, 200, 1)]
# one-hot codes: (id, B, T, Q, Nw, shift, splits); a split's 96-row blocks and
# the shift cross clip boundaries
ONEHOT_CASES = [('Q16-shift0', 3, 50, 16, 32, 0, 4), ('Q16-shift3', 3, 50, 16, 32, 3, 4),
                ('Q256-shift5', 2, 97, 256, 36, 5, 3), ('Q123-shift49-T50', 5, 50, 123, 32, 49, 1)]
