"""The GEMM entry points against float64 with operands for which float32 is
exact (tests/gemm_ref.py; the premise is proved on the CPU by
tests/test_gemm_ref_host.py): every output BIT must match, at every kernel the
host's dispatch can pick, with leading dimensions and plane strides that are
not the matrix width (inputs padded with NaN, outputs with a sentinel pattern
that must survive), with mask values at the edge of `> 0`, and with strides
that put the kernels' 32-bit byte offsets next to 2^31.  Random operands are
held to a measured yardstick instead: four times the error of a plain float32
evaluation of the same product."""
import functools

import numpy as np
import pytest
import torch

from util import PKG  # noqa: F401
import gemm_ref as R

pytestmark = pytest.mark.gpu

SEED = 20
SENT = -0x21524111                    # 0xdeadbeef as int32: a float no case computes
HUGE = 1 << 24                        # words; larger buffers get the constant sentinel


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ids(cases):
    return [c[0] for c in cases]


class In(object):
    """An input operand: `mat` at flat positions `idx` of a NaN-filled buffer."""

    def __init__(self, mat, idx=None, dtype=torch.float32):
        mat = np.ascontiguousarray(mat)
        if idx is None:
            self.buf = torch.from_numpy(mat).to(dtype).cuda()
        else:
            self.buf = torch.full((int(idx.max()) + 1,), float('nan'), device='cuda')
            self.buf[torch.from_numpy(idx.reshape(-1)).cuda()] = \
                torch.from_numpy(mat.reshape(-1)).to(dtype).cuda()
        self.ptr = self.buf.data_ptr()


class Out(object):
    """An output operand: its elements live at flat positions `idx`; every
    other word holds a sentinel that has to be there, bit for bit, afterwards."""

    def __init__(self, idx, tail=8):
        self.n = int(idx.max()) + 1 + tail
        self.idx = torch.from_numpy(idx.reshape(-1)).cuda()
        self.shape = idx.shape
        if self.n > HUGE:
            self.sent = None
            self.buf = torch.full((self.n,), SENT, dtype=torch.int32, device='cuda')
        else:
            pat = (np.arange(self.n, dtype=np.uint64) * 2654435761 + 0x9e3779b9) & 0xffffffff
            self.sent = torch.from_numpy(pat.astype(np.uint32).view(np.int32)).cuda()
            self.buf = self.sent.clone()
        self.ptr = self.buf.data_ptr()

    def check(self, want64, what):
        want = R.bits(R.exact32(want64)).reshape(-1)
        got = self.buf[self.idx].cpu().numpy().view(np.uint32)
        bad = np.nonzero(got != want)[0]
        if bad.size:
            k = int(bad[0])
            pos = np.unravel_index(k, self.shape)
            raise AssertionError('%s: %d of %d elements differ, first at %s: got %r (0x%08x), want %r (0x%08x)'
                                 % (what, bad.size, want.size, pos, got[k:k + 1].view(np.float32)[0],
                                    got[k], want[k:k + 1].view(np.float32)[0], want[k]))
        if self.sent is None:
            assert not (want == np.uint32(SENT & 0xffffffff)).any()
            written = int((self.buf != SENT).sum())
            assert written == want.size, '%s: %d padding words written' % (what, written - want.size)
        else:
            keep = torch.ones(self.n, dtype=torch.bool, device='cuda')
            keep[self.idx] = False
            assert torch.equal(self.buf[keep], self.sent[keep]), '%s: padding written' % what


@pytest.fixture
def big_memory():
    """The 2 GB cases give their buffers back before the next test."""
    yield
    torch.cuda.empty_cache()


# ---- NN ----------------------------------------------------------------------
def nn_run(o, M, N, K, what, pre64=None, bias=True, relu=1, mask=True, add=True, cpre=True,
           nprod=0, pad=False, a_planes=0, c_planes=0, add_planes=False, ld=None):
    """One wn_gemm_nn / wn_gemm_nn_split launch on operands `o`, checked bit for
    bit.  pad: every leading dimension / plane stride wider than its matrix;
    ld: dict of explicit overrides (lda, ldw, ldc, ld_mask, ld_add, aps, cps)."""
    from wavenet import _lib
    d = dict(lda=K, ldw=N, ldc=N, ld_mask=N, ld_add=N, aps=M * 32, cps=M * 32)
    if pad:
        d = dict(lda=K + 4, ldw=N + 4, ldc=N + 8, ld_mask=N + 12, ld_add=N + 4,
                 aps=M * 32 + 64, cps=M * 32 + 64)
    d.update(ld or {})
    A = In(o['A'], R.plane_index(M, K, d['aps']) if a_planes else R.dense_index(M, K, d['lda']))
    W = In(o['W'], R.dense_index(K, N, d['ldw']))
    b = In(o['bias']) if bias else None
    mk = In(o['mask'], R.dense_index(M, N, d['ld_mask'])) if mask else None
    c_idx = R.plane_index(M, N, d['cps']) if c_planes else R.dense_index(M, N, d['ldc'])
    ad = None
    if add:
        ad = In(o['add'], c_idx if add_planes else R.dense_index(M, N, d['ld_add']))
    C = Out(c_idx)
    P = Out(R.dense_index(M, N, d['ldc'])) if cpre else None
    p = lambda x: None if x is None else x.ptr
    args = (A.ptr, 0 if a_planes else d['lda'], a_planes, d['aps'] if a_planes else 0, W.ptr, d['ldw'],
            p(b), p(mk), d['ld_mask'] if mask else 0, p(ad), 0 if add_planes or not add else d['ld_add'],
            C.ptr, d['ldc'] if (cpre or not c_planes) else 0, c_planes, d['cps'] if c_planes else 0,
            p(P), M, N, K, relu)
    if nprod:
        lib = _lib.load()
        scratch = torch.empty(lib.wn_gemm_split_w_bytes(K, N) // 4, dtype=torch.int32, device='cuda')
        _lib.call('wn_gemm_nn_split', *(args + (scratch.data_ptr(), nprod, _st())))
    else:
        _lib.call('wn_gemm_nn', *(args + (_st(),)))
    if pre64 is None:
        pre64 = o['A'].astype(np.float64) @ o['W'].astype(np.float64)
    pre64 = pre64 + (o['bias'].astype(np.float64) if bias else 0.0) + 0.0
    c64 = R.nn_epilogue(pre64, relu, o['mask'] if mask else None,
                        o['add'].astype(np.float64) if add else None)
    C.check(c64, what + ' C')
    if cpre:
        P.check(pre64, what + ' Cpre')


def _kernels(K):
    return (0, 3, 6, 9) if K % 16 == 0 else (0,)


@pytest.mark.parametrize('pad', [False, True], ids=['tight', 'padded'])
@pytest.mark.parametrize('name,M,N,K', R.NN_CASES, ids=_ids(R.NN_CASES))
def test_nn_family_a(hip_lib, name, M, N, K, pad):
    """Family (a) with the whole epilogue (bias, ReLU, mask with zeros of both
    signs and tiny values, addend, pre-activation copy) on wn_gemm_nn and, where
    K % 16 == 0, wn_gemm_nn_split with 3, 6 and 9 products (the operands have one
    nonzero piece: every product set is exact)."""
    o = R.family_a_nn(M, N, K, SEED)
    for nprod in _kernels(K):
        nn_run(o, M, N, K, '%s x%d' % (name, nprod), nprod=nprod, pad=pad)
    # no epilogue at all: row exponents over all of +-20
    o = R.family_a_nn(M, N, K, SEED, epilogue=False)
    for nprod in _kernels(K):
        nn_run(o, M, N, K, '%s plain x%d' % (name, nprod), bias=False, relu=0, mask=False,
               add=False, cpre=False, nprod=nprod, pad=pad)


@pytest.mark.parametrize('pad', [False, True], ids=['tight', 'padded'])
@pytest.mark.parametrize('name,M,P,X', R.PLANE_CASES, ids=_ids(R.PLANE_CASES))
def test_nn_planes(hip_lib, name, M, P, X, pad):
    """A as P planes of [M][32] (K = 32 P) and C as P planes (N = 32 P), the
    addend dense or in C's plane layout, plane strides M * 32 and M * 32 + 64."""
    o = R.family_a_nn(M, X, 32 * P, SEED)
    for nprod in _kernels(32 * P):
        nn_run(o, M, X, 32 * P, '%s planes in x%d' % (name, nprod), nprod=nprod, pad=pad, a_planes=P)
    o = R.family_a_nn(M, 32 * P, X, SEED)
    for nprod in _kernels(X):
        for add_planes in (False, True):
            nn_run(o, M, 32 * P, X, '%s planes out x%d addp%d' % (name, nprod, add_planes),
                   nprod=nprod, pad=pad, c_planes=P, add_planes=add_planes)
    # planes in and out (the channel-block models' residual conv)
    o = R.family_a_nn(M, 32 * P, 32 * P, SEED)
    nn_run(o, M, 32 * P, 32 * P, name + ' planes in+out', pad=pad, a_planes=P, c_planes=P,
           add_planes=True, cpre=False)


@pytest.mark.parametrize('nprod', [0, 3, 6, 9], ids=['fp32', 'x3', 'x6', 'x9'])
def test_nn_every_epilogue(hip_lib, nprod):
    """All sixteen combinations of ReLU, mask, addend and Cpre, with and without
    bias, at an edge shape (ragged in M and N, three K chunks)."""
    M, N, K = R.EPILOGUE_SHAPE
    o = R.family_a_nn(M, N, K, SEED)
    for e in range(32):
        nn_run(o, M, N, K, 'epilogue %d x%d' % (e, nprod), bias=bool(e & 16), relu=e & 1,
               mask=bool(e & 2), add=bool(e & 4), cpre=bool(e & 8), nprod=nprod, pad=bool(e & 1))


_B_NN = [(k,) + c for k in R.B_KINDS for c in R.NN_B_CASES]


@pytest.mark.parametrize('kind,name,M,N,K', _B_NN, ids=['%s-%s' % c[:2] for c in _B_NN])
def test_nn_split_family_b(hip_lib, kind, name, M, N, K):
    """Family (b): operands with two or three nonzero pieces; the expected bits
    are gemm_ref's restatement of split3 and of the product sets (x3 drops the
    products it has to drop and nothing else)."""
    o = R.family_b_nn(kind, M, N, K, SEED)
    for nprod in (3, 6, 9):
        for pad in (False, True):
            nn_run(o, M, N, K, '%s %s x%d pad%d' % (kind, name, nprod, pad),
                   pre64=R.split_matmul(o['A'], o['W'], nprod), bias=False, relu=1, mask=False,
                   add=False, cpre=True, nprod=nprod, pad=pad)
    # the fp32 kernel on the same operands: the full product
    nn_run(o, M, N, K, '%s %s fp32' % (kind, name), bias=False, relu=0, mask=False, add=False)


# ---- TN ----------------------------------------------------------------------
def tn_run(A, G, rows, Mw, Nw, splits, colsum, what, ref64=None, cs64=None, pad=False,
           a_planes=0, codes=None, shift=0, T=1, nprod=0, ld=None):
    """wn_gemm_tn / wn_gemm_tn_split into NaN slabs, summed by wn_reduce_slabs
    and by wn_reduce_slabs_mt; matrix (and column sums) checked bit for bit."""
    from wavenet import _lib
    lib = _lib.load()
    d = dict(lda=Mw + 4, ldg=Nw + 4, aps=rows * 32 + 64) if pad else dict(lda=Mw, ldg=Nw, aps=rows * 32)
    d.update(ld or {})
    if codes is not None:
        dA = In(codes, dtype=torch.int32)
        a_args = (None, 0, 0, 0, dA.ptr, shift, T)
    else:
        dA = In(A, R.plane_index(rows, Mw, d['aps']) if a_planes else R.dense_index(rows, Mw, d['lda']))
        a_args = (dA.ptr, 0 if a_planes else d['lda'], a_planes, d['aps'] if a_planes else 0)
        if not nprod:
            a_args += (None, 0, 1)
    dG = In(G, R.dense_index(rows, Nw, d['ldg']))
    sl = lib.wn_gemm_tn_slab_floats(Mw, Nw)
    tr = lib.wn_gemm_tn_tail_rows(Mw, Nw)
    slabs = torch.full((splits * sl,), float('nan'), device='cuda')
    if nprod:
        _lib.call('wn_gemm_tn_split', *(a_args + (dG.ptr, d['ldg'], slabs.data_ptr(), splits, rows, Mw,
                                                  Nw, colsum, nprod, _st())))
    else:
        _lib.call('wn_gemm_tn', *(a_args + (dG.ptr, d['ldg'], slabs.data_ptr(), splits, rows, Mw, Nw,
                                            colsum, _st())))
    if ref64 is None:
        ref64, cs64 = R.tn_ref(A, G)
    if colsum != 2:
        out, cs = Out(R.dense_index(1, Mw * Nw, Mw * Nw)), Out(R.dense_index(1, Nw, Nw))
        _lib.call('wn_reduce_slabs', slabs.data_ptr(), splits, sl, 1, 0, 0, Mw * Nw, out.ptr, 0, 1, 0, _st())
        out.check(ref64.reshape(1, -1), what + ' dW (wn_reduce_slabs)')
        if colsum:
            _lib.call('wn_reduce_slabs', slabs.data_ptr(), splits, sl, 1, 0, Mw * Nw, Nw, cs.ptr, 0, 1, 0, _st())
            cs.check(cs64.reshape(1, -1), what + ' column sums (wn_reduce_slabs)')
    if (Mw * Nw) % 4 == 0 and Nw % 4 == 0:
        out, cs = Out(R.dense_index(1, Mw * Nw, Mw * Nw)), Out(R.dense_index(1, Nw, Nw))
        _lib.call('wn_reduce_slabs_mt', slabs.data_ptr(), splits, sl, Mw * Nw, out.ptr,
                  Nw if colsum else 0, cs.ptr if colsum else None, 1, Nw, tr if colsum == 2 else 1, _st())
        out.check(ref64.reshape(1, -1), what + ' dW (wn_reduce_slabs_mt)')
        if colsum:
            cs.check(cs64.reshape(1, -1), what + ' column sums (wn_reduce_slabs_mt)')
    else:
        assert colsum != 2


@pytest.mark.parametrize('pad', [False, True], ids=['tight', 'padded'])
@pytest.mark.parametrize('name,rows,Mw,Nw,splits,colsum', R.TN_CASES, ids=_ids(R.TN_CASES))
def test_tn_family_a(hip_lib, name, rows, Mw, Nw, splits, colsum, pad):
    o = R.family_a_tn(rows, Mw, Nw, SEED)
    tn_run(o['A'], o['G'], rows, Mw, Nw, splits, colsum, name, pad=pad)


@pytest.mark.parametrize('pad', [False, True], ids=['tight', 'padded'])
@pytest.mark.parametrize('name,rows,P,Nw,splits,colsum', [
    ('dma51', 96, 5, 128, 3, 1), ('dma41-raggedrows-spread', 100, 4, 128, 2, 2),
    ('wave21-ragged', 100, 2, 36, 3, 1), ('wave11-long', 1603, 1, 32, 40, 1)],
    ids=['dma51', 'dma41-raggedrows-spread', 'wave21-ragged', 'wave11-long'])
def test_tn_plane_operand(hip_lib, name, rows, P, Nw, splits, colsum, pad):
    """A as P planes of [rows][32], plane stride rows * 32 and rows * 32 + 64."""
    o = R.family_a_tn(rows, 32 * P, Nw, SEED)
    tn_run(o['A'], o['G'], rows, 32 * P, Nw, splits, colsum, name, pad=pad, a_planes=P)
    if rows % 16 == 0:
        for nprod in (3, 6, 9):
            tn_run(o['A'], o['G'], rows, 32 * P, Nw, splits, min(colsum, 1), '%s x%d' % (name, nprod),
                   pad=pad, a_planes=P, nprod=nprod)


@pytest.mark.parametrize('name,B,T,Q,Nw,shift,splits', R.ONEHOT_CASES, ids=_ids(R.ONEHOT_CASES))
def test_tn_one_hot_codes(hip_lib, name, B, T, Q, Nw, shift, splits):
    """A generated from int codes (the causal layer's weight gradient): clips of
    T rows, the codes lag `shift` rows, the first `shift` rows of a clip are
    zero; 96-row blocks and splits cross the clip boundaries."""
    rng = np.random.default_rng(SEED)
    codes = rng.integers(0, Q, B * T).astype(np.int32)
    G = R.family_a_tn(B * T, 4, Nw, SEED)['G']
    A = R.one_hot(codes, shift, T, Q)
    for pad in (False, True):
        tn_run(A, G, B * T, Q, Nw, splits, 1, '%s pad%d' % (name, pad), pad=pad, codes=codes,
               shift=shift, T=T)


@pytest.mark.parametrize('pad', [False, True], ids=['tight', 'padded'])
@pytest.mark.parametrize('name,rows,Mw,Nw,splits', R.TN_SPLIT_CASES, ids=_ids(R.TN_SPLIT_CASES))
def test_tn_split(hip_lib, name, rows, Mw, Nw, splits, pad):
    """wn_gemm_tn_split: family (a) with column sums (every product set exact),
    family (b) against the restated product sets."""
    o = R.family_a_tn(rows, Mw, Nw, SEED)
    for nprod in (3, 6, 9):
        tn_run(o['A'], o['G'], rows, Mw, Nw, splits, 1, '%s a x%d' % (name, nprod), pad=pad, nprod=nprod)
    for kind in R.B_KINDS:
        o = R.family_b_tn(kind, rows, Mw, Nw, SEED)
        for nprod in (3, 6, 9):
            want = R.split_matmul(np.ascontiguousarray(o['A'].T), o['G'], nprod)
            tn_run(o['A'], o['G'], rows, Mw, Nw, splits, 0, '%s %s x%d' % (name, kind, nprod),
                   ref64=want, pad=pad, nprod=nprod)


# ---- random operands against a measured yardstick -----------------------------
MARGIN = 4.0      # the margin the model-level tests give the float32 oracle


@functools.lru_cache(maxsize=None)
def _normal_nn(M, N, K):
    rng = np.random.default_rng([SEED, M, N, K])
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = rng.standard_normal((K, N)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    mask = rng.standard_normal((M, N)).astype(np.float32)
    return A, W, bias, mask


@functools.lru_cache(maxsize=None)
def _yard(kind, M, N, K, nprod):
    """yardstick of the problem (computed once per shape and product set)"""
    if kind == 'nn':
        A, W, bias, _ = _normal_nn(M, N, K)
        return R.yardstick(A, W, bias, nprod)
    A, G = _normal_tn(M, N, K)
    return R.yardstick(np.ascontiguousarray(A.T), G, None, nprod)


@functools.lru_cache(maxsize=None)
def _normal_tn(rows, Mw, Nw):
    rng = np.random.default_rng([SEED, rows, Mw, Nw, 1])
    return (rng.standard_normal((rows, Mw)).astype(np.float32),
            rng.standard_normal((rows, Nw)).astype(np.float32))


def _ratio(tag, err, e32):
    print('gemm_error_ratio %-44s kernel %.3e  e32 %.3e  ratio %.3f' % (tag, err, e32, err / e32))
    return err / e32


NN_NORMAL = [(1, 4, 4), (37, 16, 16), (300, 132, 68), (5000, 256, 512), (129, 512, 96),
             (256, 200, 64), (1031, 1600, 32)]
NN_SPLIT_NORMAL = [(37, 16, 16), (5000, 256, 512), (129, 512, 96), (256, 200, 64),
                   (1031, 1600, 32), (300, 72, 48)]
_NN_NORMAL = [(0,) + s for s in NN_NORMAL] + [(n,) + s for s in NN_SPLIT_NORMAL for n in (3, 6, 9)]


@pytest.mark.parametrize('nprod,M,N,K', _NN_NORMAL,
                         ids=['%s-%dx%dx%d' % (('x%d' % c[0]) if c[0] else 'fp32', c[1], c[2], c[3])
                              for c in _NN_NORMAL])
def test_nn_normal_data_within_4x_float32(hip_lib, nprod, M, N, K):
    """Standard-normal operands at the shapes of tests/test_gpu_gemm.py: the
    kernel's max error against float64 is at most 4 x e32, e32 the max error of
    gemm_ref.f32_forward (plus, for x3 / x6, the dropped-term error of the
    restated product set)."""
    from wavenet import _lib
    lib = hip_lib
    A, W, bias, mask = _normal_nn(M, N, K)
    ref0, e32 = _yard('nn', M, N, K, nprod)
    dA, dW, db, dm = In(A), In(W), In(bias), In(mask)
    C = torch.empty((M, N), device='cuda')
    Cpre = torch.empty((M, N), device='cuda')
    args = (dA.ptr, K, 0, 0, dW.ptr, N, db.ptr, dm.ptr, N, None, 0, C.data_ptr(), N, 0, 0,
            Cpre.data_ptr(), M, N, K, 1)
    if nprod:
        scratch = torch.empty(lib.wn_gemm_split_w_bytes(K, N) // 4, dtype=torch.int32, device='cuda')
        _lib.call('wn_gemm_nn_split', *(args + (scratch.data_ptr(), nprod, _st())))
    else:
        _lib.call('wn_gemm_nn', *(args + (_st(),)))
    ref = np.where(mask > 0, np.maximum(ref0, 0), 0)
    tag = 'nn %s %dx%dx%d' % ('x%d' % nprod if nprod else 'fp32', M, N, K)
    r_pre = _ratio(tag + ' Cpre', np.abs(Cpre.cpu().numpy() - ref0).max(), e32)
    r_c = _ratio(tag + ' C', np.abs(C.cpu().numpy() - ref).max(), e32)
    assert r_pre <= MARGIN and r_c <= MARGIN


TN_NORMAL = [(100, 32, 32, 3), (1000, 64, 96, 7), (5000, 160, 128, 9), (3333, 512, 256, 5),
             (777, 96, 64, 1), (4800, 160, 128, 9), (3328, 512, 256, 5), (2048, 512, 512, 3),
             (1600, 128, 128, 40), (96, 160, 256, 2)]
TN_SPLIT_NORMAL = [(96, 32, 32, 2), (4800, 160, 128, 9), (3328, 512, 256, 5), (1600, 200, 132, 3)]
_TN_NORMAL = [(0,) + s for s in TN_NORMAL] + [(n,) + s for s in TN_SPLIT_NORMAL for n in (3, 6, 9)]


@pytest.mark.parametrize('nprod,rows,Mw,Nw,splits', _TN_NORMAL,
                         ids=['%s-%dx%dx%d-s%d' % ((('x%d' % c[0]) if c[0] else 'fp32',) + c[1:])
                              for c in _TN_NORMAL])
def test_tn_normal_data_within_4x_float32(hip_lib, nprod, rows, Mw, Nw, splits):
    """The same for dW = A^T G through the slabs and wn_reduce_slabs."""
    from wavenet import _lib
    lib = hip_lib
    A, G = _normal_tn(rows, Mw, Nw)
    ref, e32 = _yard('tn', rows, Mw, Nw, nprod)
    dA, dG = In(A), In(G)
    sl = lib.wn_gemm_tn_slab_floats(Mw, Nw)
    slabs = torch.full((splits * sl,), float('nan'), device='cuda')
    out = torch.empty(Mw * Nw, device='cuda')
    if nprod:
        _lib.call('wn_gemm_tn_split', dA.ptr, Mw, 0, 0, dG.ptr, Nw, slabs.data_ptr(), splits, rows,
                  Mw, Nw, 0, nprod, _st())
    else:
        _lib.call('wn_gemm_tn', dA.ptr, Mw, 0, 0, None, 0, 1, dG.ptr, Nw, slabs.data_ptr(), splits,
                  rows, Mw, Nw, 0, _st())
    _lib.call('wn_reduce_slabs', slabs.data_ptr(), splits, sl, 1, 0, 0, Mw * Nw, out.data_ptr(), 0, 1,
              0, _st())
    tag = 'tn %s %dx%dx%d s%d' % ('x%d' % nprod if nprod else 'fp32', rows, Mw, Nw, splits)
    assert _ratio(tag, np.abs(out.cpu().numpy().reshape(Mw, Nw) - ref).max(), e32) <= MARGIN


# ---- the 2 GB edges ------------------------------------------------------------
# Large strides, tiny work: the kernels address through 32-bit byte offsets of
# buffer resources and the host decides by byte counts which kernel may run;
# which one ran is not asserted, the bits on both sides of each predicate are.
LD_MAX = 17318412                    # (31 ld + 64) * 4 <= 2^31 - 1 < (31 (ld + 4) + 64) * 4
CPS_MAX = 2 ** 29 - 1028             # c_plane_stride * 4 + 4096 <= 2^31 - 1


@pytest.mark.parametrize('M', [511, 513], ids=['M511-under-dma', 'M513-over-fallback'])
def test_nn_lda_at_2gb(hip_lib, big_memory, M):
    """lda = 2^20 floats: M * lda * 4 just under 2^31 (the LDS-DMA kernel with
    its lane offsets at the limit) and just over (the register-staged one)."""
    N, K = 68, 32
    o = R.family_a_nn(M, N, K, SEED)
    nn_run(o, M, N, K, 'lda 2^20 M %d' % M, ld=dict(lda=1 << 20))


@pytest.mark.parametrize('ldw', [(1 << 25) - 4, 1 << 25], ids=['under-dma', 'over-fallback'])
def test_nn_ldw_at_2gb(hip_lib, big_memory, ldw):
    """16 * ldw * 4 on both sides of 2^31 (a 16-row weight chunk)."""
    M, N, K = 129, 68, 16
    o = R.family_a_nn(M, N, K, SEED)
    nn_run(o, M, N, K, 'ldw %d' % ldw, ld=dict(ldw=ldw))


@pytest.mark.parametrize('which', ['ldc', 'cpre', 'ld_mask', 'ld_add', 'c_plane_stride',
                                   'c_plane_stride-plane-addend'])
def test_nn_epilogue_strides_last_accepted(hip_lib, big_memory, which):
    """The largest leading dimension / plane stride the argument checks accept
    (tests/test_gemm_ref_host.py refuses the next): rows 31 and 32 lie 2 GB
    from row 0 and every one of them is computed and stored."""
    M, N, K = 33, 64, 16
    o = R.family_a_nn(M, N, K, SEED)
    if which == 'ldc':
        nn_run(o, M, N, K, which, cpre=False, ld=dict(ldc=LD_MAX))
    elif which == 'cpre':
        nn_run(o, M, N, K, which, c_planes=2, add_planes=True, ld=dict(ldc=LD_MAX))
    elif which == 'ld_mask':
        nn_run(o, M, N, K, which, ld=dict(ld_mask=LD_MAX))
    elif which == 'ld_add':
        nn_run(o, M, N, K, which, ld=dict(ld_add=LD_MAX))
    elif which == 'c_plane_stride':
        nn_run(o, M, N, K, which, c_planes=2, ld=dict(cps=CPS_MAX))
    else:
        nn_run(o, M, N, K, which, c_planes=2, add_planes=True, cpre=False, ld=dict(cps=CPS_MAX))


# a split's rows + 96, times the row bytes, against 2^31 (wn_gemm_tn's `dma`)
TN_ROWS = 192
TN_LD_UNDER = (1 << 29) // (TN_ROWS + 96) // 4 * 4               # 1864132
TN_APS_UNDER = ((1 << 29) - (TN_ROWS + 96) * 32) // 5 // 4 * 4   # 107372336


@pytest.mark.parametrize('which,ld', [
    ('lda', TN_LD_UNDER), ('lda', TN_LD_UNDER + 4), ('ldg', TN_LD_UNDER), ('ldg', TN_LD_UNDER + 4),
    ('aps', TN_APS_UNDER), ('aps', TN_APS_UNDER + 4)],
    ids=['lda-under-dma', 'lda-over-fallback', 'ldg-under-dma', 'ldg-over-fallback',
         'planes-under-dma', 'planes-over-fallback'])
def test_tn_strides_at_2gb(hip_lib, big_memory, which, ld):
    """Tile-aligned outputs, splits = 1: (rows + 96) * ld * 4 (dense) and
    (5 * plane stride + (rows + 96) * 32) * 4 (planes) on both sides of 2^31."""
    rows = TN_ROWS
    assert (rows + 96) * TN_LD_UNDER * 4 < 2 ** 31 <= (rows + 96) * (TN_LD_UNDER + 4) * 4
    assert (5 * TN_APS_UNDER + (rows + 96) * 32) * 4 < 2 ** 31 <= (5 * (TN_APS_UNDER + 4) + (rows + 96) * 32) * 4
    if which == 'aps':
        o = R.family_a_tn(rows, 160, 128, SEED)
        tn_run(o['A'], o['G'], rows, 160, 128, 1, 1, '%s %d' % (which, ld), a_planes=5, ld=dict(aps=ld))
    else:
        o = R.family_a_tn(rows, 128, 128, SEED)
        tn_run(o['A'], o['G'], rows, 128, 128, 1, 2, '%s %d' % (which, ld), ld={which: ld})
