"""Every entry of the C ABI on its own, its operands inside guard bands
(tests/guard.py): no launch writes outside an operand (`check`), and no output
depends on what lies outside an input (`read_check`: bands NaN / Q - 1, then
0.0 / 0, equal output bits).  Values are NOT re-asserted here; the parity
tests do that.

Table driven: a Row names the entry, the builder that places its operands in
an arena and returns the calls, and the entry's smallest edge shapes -- those
of its parity test plus remainder 1 and tile - 1 of every tile constant the
kernel source names (cited beside the cases).  Leading dimensions are larger
than the width wherever the entry takes one (the gap columns are band), and
plane strides larger than rows * 32 wherever it takes one, so every plane has
bands of its own.  A row with `skew` runs once more with that operand 4 bytes
off its 256-byte alignment: where the entry documents 4-byte alignment the
call must pass both checks again, where it documents WN_ERR_MISALIGNED it must
return that code and leave every band and every operand untouched.

EXEMPT: entries that write through a pointer and have no row, each with its
reason.  tests/test_guard_host.py holds include/wavenet_hip.h against ROWS and
EXEMPT, so a new entry cannot arrive unguarded."""
import collections

import numpy as np
import pytest
import torch

import guard

pytestmark = pytest.mark.gpu

F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64
PLANE_PAD = 1024          # floats between the planes of one operand: a 32-row tile
LAYER_BLOCK = 5216        # LAYER_BLOCK_FLOATS (wn_common.h): 5 * 1024 + 96
WN_ERR_UNSUPPORTED, WN_ERR_MISALIGNED = -2, -3

Row = collections.namedtuple('Row', 'entry build cases skew')


def pstride(rows):
    return rows * 32 + PLANE_PAD


class Ctx(object):
    """The arena of one case and the shorthand the builders place with."""

    def __init__(self, lib, skew=None, device='cuda'):
        self.lib, self.skew = lib, skew
        self.a = guard.Arena(device)
        self.rng = np.random.default_rng(7)
        self.st = torch.cuda.current_stream().cuda_stream \
            if self.a.device.type == 'cuda' else None
        self.host = []                   # host arrays the calls point into
        self.expect = 0                  # the code the calls must return

    def _sk(self, name):
        return 4 if name == self.skew else 0

    def fin(self, name, shape, ld=None, role='in', kind='normal', scale=1.0,
            tile_ld=None, fill=None, dtype=F32):
        """float operand with random contents: 'normal', 'pos' (0.1 .. 1.1:
        second moments, sigmoid planes), 'unit' (-1 .. 1: audio)"""
        if isinstance(shape, int):
            shape = (shape,)
        if kind == 'normal':
            d = self.rng.standard_normal(shape) * scale
        elif kind == 'pos':
            d = self.rng.uniform(0.1, 0.9, shape) * scale
        else:
            d = self.rng.uniform(-1, 1, shape)
        np_dt = np.float64 if dtype == F64 else np.float32
        return self.a.place(name, d.astype(np_dt), dtype, ld=ld, role=role,
                            skew_bytes=self._sk(name), fill=fill,
                            tile_ld=tile_ld).data_ptr()

    def out(self, name, shape, dtype=F32, ld=None, tile_ld=None, fill=None):
        if isinstance(shape, int):
            shape = (shape,)
        return self.a.place(name, tuple(shape), dtype, ld=ld, role='out',
                            skew_bytes=self._sk(name), fill=fill,
                            tile_ld=tile_ld).data_ptr()

    def ints(self, name, data, fill, role='in', dtype=I32):
        """an operand whose values become indices: both fills in range"""
        return self.a.place(name, np.asarray(data), dtype, role=role,
                            skew_bytes=self._sk(name), fill=fill).data_ptr()

    def codes(self, name, n, Q):
        return self.ints(name, self.rng.integers(0, Q, n), (Q - 1, 0))

    def planes(self, name, P, rows, role='in', kind='normal', scale=1.0):
        """P planes of [rows][32], pstride(rows) floats apart"""
        if role == 'out':
            return self.out(name, (P, rows * 32), ld=pstride(rows), tile_ld=32)
        return self.fin(name, (P, rows * 32), ld=pstride(rows), role=role,
                        kind=kind, scale=scale, tile_ld=32)

    def host_array(self, values, dtype):
        a = np.ascontiguousarray(values, dtype=dtype)
        self.host.append(a)
        return a.ctypes.data


def run_calls(c, calls):
    for name, args in calls:
        code = getattr(c.lib, name)(*args)
        if code != 0:
            return code
    return 0


# ============================================================ GEMMs, sums
def b_gemm_nn(c, M, N, K, mode='dense', relu=0, mask=0, add=0, pre=1,
              nprod=0):
    """wn_gemm_nn / wn_gemm_nn_split (nprod): dense operands with every
    leading dimension padded, or planes with padded strides"""
    lda, ldw, ldc, ldm, ldadd = K + 4, N + 4, N + 8, N + 4, N + 12
    a_planes = c_planes = 0
    a_ps = c_ps = 0
    if mode in ('a_planes', 'plane_add'):
        a_planes, a_ps, lda = K // 32, pstride(M), 0
        A = c.planes('A', a_planes, M)
    else:
        A = c.fin('A', (M, K), ld=lda)
    W = c.fin('W', (K, N), ld=ldw)
    bias = c.fin('bias', N)
    pm = c.fin('mask', (M, N), ld=ldm) if mask else None
    padd, Cpre = None, None
    if mode in ('c_planes', 'plane_add'):
        c_planes, c_ps, ldc = N // 32, pstride(M), 0
        if add or mode == 'plane_add':
            padd, ldadd = c.planes('addend', c_planes, M), 0
        C = c.planes('C', c_planes, M, role='out')
    else:
        if add:
            padd = c.fin('addend', (M, N), ld=ldadd)
        C = c.out('C', (M, N), ld=ldc)
        if pre:
            Cpre = c.out('Cpre', (M, N), ld=ldc)
    args = (A, lda, a_planes, a_ps, W, ldw, bias, pm, ldm, padd, ldadd, C,
            ldc, c_planes, c_ps, Cpre, M, N, K, relu)
    if nprod:
        ws = c.out('w_scratch', c.lib.wn_gemm_split_w_bytes(K, N) // 4, I32)
        return [('wn_gemm_nn_split', args + (ws, nprod, c.st))]
    return [('wn_gemm_nn', args + (c.st,))]


_EPI = [dict(), dict(relu=1), dict(mask=1), dict(relu=1, add=1)]
# NN_TM = NN_TN = 128 (wn_gemm.hip): M, N at remainder 1 and 127; N % 128 in
# {32, 64}: a wave half beyond N; N3_KC = 16: K % 16 != 0 takes the
# register-staged gemm_nn_kernel<2>, K chunks of NN_KC = 32
NN_CASES = [dict(M=M, N=N, K=K, **e) for M, N, K in
            [(1, 4, 4), (37, 16, 16), (129, 132, 68), (127, 160, 96),
             (257, 192, 64), (300, 256, 20)] for e in _EPI] + [
    dict(M=129, N=64, K=160, mode='a_planes'),
    dict(M=777, N=64, K=160, mode='a_planes', relu=1, pre=1),
    dict(M=129, N=160, K=48, mode='c_planes'),          # N % 128 == 32
    dict(M=300, N=192, K=48, mode='c_planes', add=1),   # N % 128 == 64
    dict(M=1, N=32, K=16, mode='c_planes'),
    dict(M=300, N=64, K=64, mode='plane_add'),
    dict(M=129, N=256, K=256, mode='plane_add'),
]
# S16_KC = 32: K = 16, 48 leave the last chunk half empty
NN_SPLIT_CASES = [dict(M=M, N=N, K=K, nprod=p, relu=1, mask=1) for M, N, K, p in
                  [(37, 16, 16, 6), (129, 160, 96, 6), (257, 192, 48, 9),
                   (300, 72, 48, 3)]] + [
    dict(M=129, N=160, K=64, mode='c_planes', nprod=6),
    dict(M=129, N=64, K=160, mode='a_planes', nprod=6)]


def b_gemm_tn(c, rows, Mw, Nw, colsum=1, planes=0, onehot=None, nprod=0,
              splits=0):
    """wn_gemm_tn / wn_gemm_tn_split: the slab count from wn_gemm_tn_splits,
    slabs with the column-sum tail rows"""
    lib = c.lib
    lda, ldg = Mw + 4, Nw + 4
    G = c.fin('G', (rows, Nw), ld=ldg)
    A, codes, shift, T = None, None, 0, 1
    a_planes = a_ps = 0
    if onehot:
        B, T, shift = onehot
        assert B * T == rows
        codes, lda = c.codes('codes', rows, Mw), 0
    elif planes:
        a_planes, a_ps, lda = planes, pstride(rows), 0
        A = c.planes('A', planes, rows)
    else:
        A = c.fin('A', (rows, Mw), ld=lda)
    kind = 2 if nprod else 1 if onehot else 0
    sp = splits or lib.wn_gemm_tn_splits(rows, Mw, Nw, kind)
    sl = lib.wn_gemm_tn_slab_floats(Mw, Nw)
    assert sl == Mw * Nw + lib.wn_gemm_tn_tail_rows(Mw, Nw) * Nw
    slabs = c.out('slabs', (sp, sl))
    if nprod:
        return [('wn_gemm_tn_split', (A, lda, a_planes, a_ps, G, ldg, slabs,
                                      sp, rows, Mw, Nw, colsum, nprod, c.st))]
    return [('wn_gemm_tn', (A, lda, a_planes, a_ps, codes, shift, T, G, ldg,
                            slabs, sp, rows, Mw, Nw, colsum, c.st))]


# rows_per_split is rounded to 96 rows (32-row chunks, 6 / 8-row groups):
# rows at 96 k + 1 and 96 k - 1; tn_wg_tile: Mw % 160 / 128, Nw % 256 / 128
# take the LDS-staged kernels (rows % 16 == 0: gemm_tn3, else gemm_tn2), every
# other shape gemm_tn_kernel<MF, NF> on 32 x 32 wave tiles
TN_CASES = [
    dict(rows=100, Mw=32, Nw=32, splits=3), dict(rows=1, Mw=4, Nw=4),
    dict(rows=97, Mw=64, Nw=96, colsum=0), dict(rows=1000, Mw=64, Nw=96),
    dict(rows=777, Mw=96, Nw=64), dict(rows=95, Mw=100, Nw=36, splits=2),
    dict(rows=193, Mw=20, Nw=132),
    dict(rows=96, Mw=160, Nw=256, splits=2),
    dict(rows=1600, Mw=128, Nw=128), dict(rows=1600, Mw=256, Nw=128, colsum=2),
    dict(rows=1031, Mw=160, Nw=128), dict(rows=1031, Mw=320, Nw=128, colsum=2),
    dict(rows=1537, Mw=256, Nw=256, colsum=2, splits=5),
    dict(rows=1000, Mw=160, Nw=128, planes=5),
    dict(rows=1600, Mw=320, Nw=128, planes=10, colsum=2),
    dict(rows=333, Mw=64, Nw=32, planes=2),
    dict(rows=150, Mw=16, Nw=32, onehot=(3, 50, 1), colsum=0),
    dict(rows=150, Mw=16, Nw=32, onehot=(3, 50, 3), colsum=0, splits=4),
    dict(rows=1665, Mw=123, Nw=32, onehot=(5, 333, 0), colsum=0),
    dict(rows=1, Mw=256, Nw=32, onehot=(1, 1, 0), colsum=0),
]
# 128 x 128 tiles, rows % 16 == 0 (else refused)
TN_SPLIT_CASES = [dict(rows=96, Mw=32, Nw=32, nprod=6, splits=2),
                  dict(rows=1600, Mw=200, Nw=132, nprod=6),
                  dict(rows=4800, Mw=160, Nw=128, nprod=9, planes=5),
                  dict(rows=16, Mw=132, Nw=4, nprod=3)]


def b_reduce_slabs(c, ns, n, batch=1, rep=1, stride=None, off=0):
    stride = stride or n + 3
    bstride = ns * stride + 5 if batch > 1 else 0
    obs = n + 4 if batch > 1 else 0
    rstride = batch * (n + 4) + 8 if rep > 1 else 0
    if (stride | off | n) % 4 == 0:      # keep the 16-byte path's strides
        bstride, obs, rstride = [(x + 3) // 4 * 4
                                 for x in (bstride, obs, rstride)]
    src = c.fin('slabs', (batch - 1) * bstride + off + (ns - 1) * stride + n)
    dst = c.out('dst', (batch - 1) * obs + (rep - 1) * rstride + n)
    return [('wn_reduce_slabs', (src, ns, stride, batch, bstride, off, n, dst,
                                 obs, rep, rstride, c.st))]


# n <= 4 with >= 256 slabs: the wave kernel; everything a multiple of 4:
# reduce_slabs4_kernel (<4> from 32 slabs on, 64 float4 per workgroup); else
# the scalar kernel (256 per workgroup)
REDUCE_CASES = [dict(ns=1026, n=1), dict(ns=300, n=3, batch=2, rep=2, off=2),
                dict(ns=255, n=2), dict(ns=256, n=4, batch=3),
                dict(ns=40, n=64, stride=68), dict(ns=3, n=1028, stride=1032,
                                                   batch=2, off=4),
                dict(ns=31, n=260, stride=264, rep=2),
                dict(ns=5, n=1025), dict(ns=1, n=257, batch=2, rep=2),
                dict(ns=7, n=1)]


def b_reduce_slabs_mt(c, ns, n_main, n_tail, rep=1, tail_rows=1):
    stride = n_main + tail_rows * n_tail + 8
    src = c.fin('slabs', (ns, n_main + tail_rows * n_tail), ld=stride)
    dm = c.out('dst_main', n_main)
    rstride = n_tail + 4
    dt = c.out('dst_tail', (rep, n_tail), ld=rstride) if n_tail else None
    return [('wn_reduce_slabs_mt', (src, ns, stride, n_main, dm, n_tail, dt,
                                    rep, rstride, tail_rows, c.st))]


# 64 float4 per workgroup, RMT_PARTS = 4 parts of the slabs
MT_CASES = [dict(ns=25, n_main=4096, n_tail=64),
            dict(ns=96, n_main=1024, n_tail=32, rep=5),
            dict(ns=3, n_main=64, n_tail=0), dict(ns=1, n_main=4, n_tail=4),
            dict(ns=5, n_main=260, n_tail=128, rep=2, tail_rows=4),
            dict(ns=4, n_main=252, n_tail=8, tail_rows=2)]


def b_reduce_pair_slabs(c, CB, K, dense, ub, ns=37, tap0=0, Ktot=None):
    Ktot = Ktot or K
    C = 32 * CB
    WF = (2 * K + 1) * 1024
    src = c.fin('slabs', (CB * CB * ns, WF + 96))
    off_b = (2 * Ktot + 1) * C * C
    g = c.fin('layer_grad', off_b + 3 * C, role='inout')
    return [('wn_reduce_pair_slabs', (src, ns, CB, K, dense, ub, g, C, off_b,
                                      tap0, Ktot, c.st))]


PAIR_CASES = [dict(CB=2, K=2, dense=1, ub=1), dict(CB=3, K=3, dense=0, ub=1),
              dict(CB=2, K=4, dense=1, ub=0, ns=1),
              dict(CB=2, K=2, dense=0, ub=0, tap0=3, Ktot=7)]


def b_transpose(c, rows, cols):
    in_ld, out_ld = cols + 3, rows + 5
    src = c.fin('in', (rows, cols), ld=in_ld)
    dst = c.out('out', (cols, rows), ld=out_ld)
    return [('wn_transpose', (src, rows, cols, in_ld, dst, out_ld, c.st))]


# 32 x 32 LDS tiles
TRANSPOSE_CASES = [dict(rows=1, cols=1), dict(rows=33, cols=31),
                   dict(rows=31, cols=65), dict(rows=64, cols=96),
                   dict(rows=37, cols=129)]


def b_diag(c, blocks, iters):
    out = c.out('out', blocks * 256)
    return [('wn_diag_mfma_peak', (out, blocks, iters, c.st))]


# ================================================================ layers
def _wblock(c, name, K=2, C=32):
    return c.fin(name, (2 * K + 1) * C * C + 3 * C, scale=0.2)


def b_layer_fwd(c, B, T, d, save_ts, dense=1, K=0, bias=1):
    """wn_layer_fwd (K = 0) / wn_layer_fwd_k"""
    N = B * T
    x = c.fin('x', (N, 32))
    xo = c.out('x_out', (N, 32)) if dense else None
    z = c.out('z', (N, 32))
    th = c.out('th', (N, 32)) if save_ts == 1 else None
    sg = c.out('sg', (N, 32)) if save_ts else None
    w = _wblock(c, 'wblock', K or 2)
    bfg = c.fin('bias_fg', (B, 64)) if bias else None
    args = (x, xo, z, th, sg, w, bfg, 64 if bias else 0, B, T, d)
    if K:
        return [('wn_layer_fwd_k', args + (K, dense, save_ts, c.st))]
    return [('wn_layer_fwd', args + (dense, save_ts, c.st))]


# 32-row tiles, LAYER_WAVES = 16 / GEN_WAVES = 8 / B2_WAVES = 8 tiles per
# workgroup: B * T and T at remainder 1 and 31 of 32, a clip shorter than
# the dilation, more than one workgroup
_BTD = [(1, 1, 1), (3, 33, 2), (3, 33, 64), (2, 159, 8), (3, 129, 128),
        (5, 333, 4)]
LAYER_FWD_CASES = [dict(B=B, T=T, d=d, save_ts=s) for B, T, d in _BTD
                   for s in (0, 1, 2)] + [
    dict(B=3, T=33, d=2, save_ts=2, dense=0, bias=0)]
LAYER_FWD_K_CASES = [dict(B=B, T=T, d=d, save_ts=s, K=K) for B, T, d in _BTD
                     for s, K in ((0, 3), (1, 3))] + [
    dict(B=3, T=33, d=2, save_ts=1, K=8, dense=0, bias=0),
    dict(B=2, T=159, d=8, save_ts=1, K=2)]


def b_layer_bwd2(c, B, T, d, dxin=1, colsum=1):
    lib = c.lib
    N = B * T
    layer = c.fin('wblock', LAYER_BLOCK, scale=0.2)
    wimg = c.out('wimg', lib.wn_layer_bwd2_wimg_floats())
    assert lib.wn_layer_bwd2_pack(layer, LAYER_BLOCK, wimg, 1, c.st) == 0
    torch.cuda.synchronize()
    c.a.ops['wimg'].role = 'in'          # an input from here on
    c.a.commit('wimg')
    x, z = c.fin('x', (N, 32)), c.fin('z', (N, 32), scale=0.3)
    sg = c.fin('sg', (N, 32), kind='pos')
    dZ = c.fin('dZ', (N, 32))
    pdx = c.fin('dxin', (N, 32)) if dxin else None
    dxo = c.out('dx_out', (N, 32))
    ns = lib.wn_layer_bwd2_slabs(B, T)
    slabs = c.out('slabs', (ns, lib.wn_layer_wgrad_slab_floats()))
    tcs = c.out('tile_colsum', (B * ((T + 31) // 32), 64)) if colsum else None
    return [('wn_layer_bwd2', (x, z, sg, dZ, pdx, dxo, layer, wimg, slabs,
                               tcs, B, T, d, c.st))]


LAYER_BWD2_CASES = [dict(B=B, T=T, d=d, dxin=i % 2, colsum=(i + 1) % 3 > 0)
                    for i, (B, T, d) in enumerate(_BTD)] + [
    dict(B=3, T=33, d=2), dict(B=5, T=333, d=4)]


def b_layer_bwd2_pack(c, L):
    stride = LAYER_BLOCK + 32
    layer = c.fin('layer0', (L, LAYER_BLOCK), ld=stride)
    wimg = c.out('wimg', L * c.lib.wn_layer_bwd2_wimg_floats())
    return [('wn_layer_bwd2_pack', (layer, stride, wimg, L, c.st))]


def b_stack_pack(c, L, which=3):
    stride = LAYER_BLOCK + 32
    layer = c.fin('layer0', (L, LAYER_BLOCK), ld=stride)
    n = L * c.lib.wn_stack_wimg_floats()
    wf = c.out('wimg_fwd', n) if which & 1 else None
    wb = c.out('wimg_bwd', n) if which & 2 else None
    return [('wn_stack_pack', (layer, stride, wf, wb, L, c.st))]


def b_stack_skip_pack(c, L):
    w = c.fin('skip_w', (L * 32, 512))
    img = c.out('img', c.lib.wn_stack_skip_img_floats(L))
    return [('wn_stack_skip_pack', (w, L, img, c.st))]


def b_layer_bwd_k(c, B, T, d, K, mode):
    """wn_layer_bwd_k: 'ba' phase B of a layer and phase A of the one below,
    'b' / 'a' alone, 'a2': the gate gradients of two channel blocks"""
    N = B * T
    st = c.st
    if mode == 'a2':
        ps = pstride(N)
        dZ, th = c.planes('dZ', 2, N), c.planes('th', 2, N, scale=0.5)
        sg = c.planes('sg', 2, N, kind='pos')
        w = _wblock(c, 'wblock_a', K, 64)
        f, g = c.planes('daf_next', 2, N, 'out'), c.planes('dag_next', 2, N,
                                                          'out')
        return [('wn_layer_bwd_k', (None, None, None, None, None, dZ, th, sg,
                                    w, f, g, B, T, d, K, 0, 1, 2, ps, st))]
    do_b, do_a = 'b' in mode, 'a' in mode
    daf = dag = dxin = dxo = wb = dZ = th = sg = wa = fn = gn = None
    if do_b:
        daf, dag = c.fin('daf_cur', (N, 32)), c.fin('dag_cur', (N, 32))
        dxin = c.fin('dxin', (N, 32)) if mode != 'b' else None
        dxo = c.out('dx_out', (N, 32))
        wb = _wblock(c, 'wblock_b', K)
    if do_a:
        dZ, th = c.fin('dZ', (N, 32)), c.fin('th', (N, 32), scale=0.5)
        sg = c.fin('sg', (N, 32), kind='pos')
        wa = _wblock(c, 'wblock_a', K)
        fn, gn = c.out('daf_next', (N, 32)), c.out('dag_next', (N, 32))
    return [('wn_layer_bwd_k', (daf, dag, dxin, dxo, wb, dZ, th, sg, wa, fn,
                                gn, B, T, d, K, int(do_b), int(do_a), 1, 0,
                                st))]


LAYER_BWD_K_CASES = [dict(B=B, T=T, d=d, K=3, mode=m)
                     for (B, T, d), m in zip(_BTD, ('ba', 'ba', 'b', 'a', 'ba',
                                                    'ba'))] + [
    dict(B=3, T=33, d=2, K=2, mode='a2'), dict(B=2, T=159, d=8, K=2, mode='a2'),
    dict(B=3, T=33, d=2, K=8, mode='ba')]


def b_layer_wgrad_k(c, B, T, d, K, CB=1, dense=1, ns=3, k0=0, Ktot=None):
    N = B * T
    Ktot = Ktot or K
    ps = pstride(N) if CB > 1 else 0

    def pl(name, **kw):
        return c.planes(name, CB, N, **kw) if CB > 1 else \
            c.fin(name, (N, 32), **{k: v for k, v in kw.items()})
    x, daf, dag = pl('x'), pl('daf'), pl('dag')
    z = pl('z', scale=0.3) if dense else None
    dxin = pl('dxin') if dense else None
    slabs = c.out('slabs', (CB * CB * ns, (2 * K + 1) * 1024 + 96))
    return [('wn_layer_wgrad_k', (x, daf, dag, z, dxin, slabs, ns, B, T, d, K,
                                  k0, Ktot, CB, ps, c.st))]


# CB 1: layer_wgrad_kernel (K = 2) / layer_wgrad_gen_kernel; CB 2 and 4 with
# two taps: layer_wgrad_cbn_kernel; CB 3, or more taps: per block pair
WGRAD_K_CASES = [dict(B=3, T=33, d=2, K=2), dict(B=1, T=1, d=1, K=2, ns=1),
                 dict(B=2, T=159, d=8, K=3), dict(B=3, T=33, d=64, K=3,
                                                  dense=0),
                 dict(B=3, T=33, d=2, K=2, CB=2),
                 dict(B=2, T=159, d=8, K=2, CB=2, dense=0, ns=5),
                 dict(B=3, T=129, d=4, K=2, CB=4, ns=2),
                 dict(B=3, T=33, d=2, K=2, CB=3),
                 dict(B=3, T=33, d=2, K=3, CB=2),
                 dict(B=3, T=33, d=2, K=2, CB=2, dense=0, k0=3, Ktot=7)]


def _chunks(CB, K):                      # wavenet/blocked.py
    per_k = min(K, 8)
    per_b = max(1, 8 // per_k)
    return [(k0, min(per_k, K - k0), i0, min(per_b, CB - i0))
            for k0 in range(0, K, per_k) for i0 in range(0, CB, per_b)]


def b_layer_fwd_blk(c, B, T, d, K, CB, save_ts=1, bias=1):
    """one layer of a channel-block model as wavenet/blocked.py launches it:
    all output blocks per launch, input blocks / taps in chunks chained
    through the partial pre-activation planes"""
    N, C = B * T, 32 * CB
    ps = pstride(N)
    x = c.a.place('x', c.rng.standard_normal((CB, N * 32)).astype(np.float32),
                  F32, ld=ps, tile_ld=32)
    z = c.planes('z', CB, N, 'out')
    th = c.planes('th', CB, N, 'out') if save_ts else None
    sg = c.planes('sg', CB, N, 'out') if save_ts else None
    wf = c.a.place('wf', (c.rng.standard_normal((K * C, C)) * 0.2)
                   .astype(np.float32), F32)
    wg = c.a.place('wg', (c.rng.standard_normal((K * C, C)) * 0.2)
                   .astype(np.float32), F32)
    bf = c.fin('bias_f', C) if bias else None
    bg = c.fin('bias_g', C) if bias else None
    chunks = _chunks(CB, K)
    pre = c.planes('pre', 2 * CB, N, 'out') if len(chunks) > 1 else None
    calls = []
    for ci, (k0, nk, i0, nb) in enumerate(chunks):
        last = ci == len(chunks) - 1
        wo = (k0 * C + i0 * 32) * C
        calls.append(('wn_layer_fwd_blk', (
            x.data_ptr() + 4 * i0 * ps, ps, nb, z, th, sg,
            wf.data_ptr() + 4 * wo, wg.data_ptr() + 4 * wo, C, bf, bg, 0, B,
            T, d, nk, save_ts, C, pre if ci > 0 else None,
            None if last else pre, ps, k0, K, CB, ps, c.st)))
    return calls


def b_layer_bwd_blk(c, B, T, d, K, CB, dxin=1):
    N, C = B * T, 32 * CB
    M = C * C
    ps = pstride(N)
    daf = c.a.place('daf', c.rng.standard_normal((CB, N * 32))
                    .astype(np.float32), F32, ld=ps, tile_ld=32)
    dag = c.a.place('dag', c.rng.standard_normal((CB, N * 32))
                    .astype(np.float32), F32, ld=ps, tile_ld=32)
    pdx = c.planes('dxin', CB, N) if dxin else None
    dxo = c.planes('dx_out', CB, N, 'out')
    wf = c.a.place('wf', (c.rng.standard_normal((K * C, C)) * 0.2)
                   .astype(np.float32), F32)
    wg = c.a.place('wg', (c.rng.standard_normal((K * C, C)) * 0.2)
                   .astype(np.float32), F32)
    calls = []
    for ci, (k0, nk, j0, nb) in enumerate(_chunks(CB, K)):
        src = dxo if ci > 0 else pdx
        wo = k0 * M + j0 * 32
        calls.append(('wn_layer_bwd_blk', (
            daf.data_ptr() + 4 * j0 * ps, dag.data_ptr() + 4 * j0 * ps, ps,
            nb, src, dxo, wf.data_ptr() + 4 * wo, wg.data_ptr() + 4 * wo, C,
            M, B, T, d, nk, k0, K, CB, ps, c.st)))
    return calls


# K * blocks <= 8 per call: (K 2, CB 2 / 4) one call with out_blocks /
# dx_blocks > 1; (K 3, CB 4) and (K 9, CB 2): chunks chained through
# pre_in / pre_out and dxin / dx_out
BLK_CASES = [dict(B=3, T=33, d=2, K=2, CB=2), dict(B=1, T=1, d=1, K=2, CB=2),
             dict(B=2, T=159, d=8, K=2, CB=4), dict(B=3, T=33, d=64, K=3, CB=4),
             dict(B=3, T=129, d=4, K=9, CB=2), dict(B=3, T=33, d=2, K=3, CB=3)]


def b_dense_planes(c, rows, C, bias=1, add=1, gate=0):
    CB = C // 32
    ps = pstride(rows)
    x = c.planes('in', CB, rows)
    W = c.fin('W', (C, C), scale=0.2)
    padd = c.planes('addend', CB, rows) if add else None
    if gate:
        th = c.planes('th', CB, rows, scale=0.5)
        sg = c.planes('sg', CB, rows, kind='pos')
        daf = c.planes('daf', CB, rows, 'out')
        dag = c.planes('dag', CB, rows, 'out')
        return [('wn_dense_planes_gate', (x, ps, W, padd, ps, th, sg, ps, daf,
                                          dag, ps, rows, C, c.st))]
    b = c.fin('bias', C) if bias else None
    out = c.planes('out', CB, rows, 'out')
    return [('wn_dense_planes', (x, ps, W, b, padd, ps, out, ps, rows, C,
                                 c.st))]


# a wave per 32-row tile, four per workgroup: rows at remainder 1 and 31 of
# 32 and of 128
DENSE_CASES = [dict(rows=r, C=C) for C in (64, 96, 128)
               for r in (1, 77, 129, 255)] + [
    dict(rows=33, C=32, bias=0, add=0), dict(rows=159, C=64, bias=0)]


# ===================================================== causal layer, loss
def b_causal_gather(c, B, T, Q, K):
    ldw = 64
    q = c.codes('q', B * T, Q)
    Wc = c.fin('Wc', (K * Q, 32), ld=ldw)
    x0 = c.out('x0', (B * T, 32))
    return [('wn_causal_gather', (q, Wc, x0, B, T, Q, K, ldw, c.st))]


_BTQ = [(1, 1, 256), (3, 50, 16), (5, 333, 123), (2, 129, 256), (2, 700, 256)]


def b_causal_wgrad(c, B, T, Q):
    ns = c.lib.wn_causal_wgrad_slabs(B * T)
    q = c.codes('q', B * T, Q)
    dx0 = c.fin('dx0', (B * T, 32))
    slabs = c.out('slabs', (ns, 2 * Q * 32))
    return [('wn_causal_wgrad', (q, dx0, slabs, ns, B, T, Q, c.st))]


def b_scalar_causal_fwd(c, B, T, K0):
    ldw = 64
    a = c.fin('audio', B * T, kind='unit')
    W = c.fin('W', (K0, 32), ld=ldw)
    x0 = c.out('x0', (B * T, 32))
    return [('wn_scalar_causal_fwd', (a, W, ldw, x0, B, T, K0, c.st))]


def b_scalar_causal_wgrad(c, B, T, K0, splits=3):
    a = c.fin('audio', B * T, kind='unit')
    dx0 = c.fin('dx0', (B * T, 32))
    slabs = c.out('slabs', (splits, K0 * 32))
    return [('wn_scalar_causal_wgrad', (a, dx0, slabs, splits, B, T, K0,
                                        c.st))]


# (K0 > 32: one pass over the rows per 32 taps)
SCALAR_CASES = [dict(B=1, T=1, K0=4), dict(B=3, T=50, K0=4),
                dict(B=2, T=129, K0=32), dict(B=5, T=333, K0=3),
                dict(B=3, T=33, K0=40)]


def b_xent(c, B, T, Q, kind, inplace=0, quirk=0, row_nll=1, lengths=1):
    """wn_xent / _masked / _window / _score / _score_window with ld > Q, the
    partials and the scratch sized by their count queries"""
    lib = c.lib
    N = B * T
    ld = (Q + 3) // 4 * 4 + 4
    if Q % 4:
        c.expect = WN_ERR_UNSUPPORTED    # before any launch
    if inplace:
        logits = dlog = c.fin('logits', (N, Q), ld=ld, role='inout')
    else:
        logits = c.fin('logits', (N, Q), ld=ld)
    q = c.codes('q', N, Q)
    n = np.append(c.rng.integers(1, T + 1, B - 1), T)
    if kind in ('score', 'score_window'):
        plen = c.ints('lengths', n, (T, 0)) if lengths else None
        rn = c.out('row_nll', N) if row_nll else None
        cn = c.out('clip_nll', B, F64)
        cc, ch = c.out('clip_count', B, I32), c.out('clip_correct', B, I32)
        sc = c.out('scratch', lib.wn_xent_score_scratch_floats(N))
        if kind == 'score':
            return [('wn_xent_score', (logits, ld, q, plen, rn, cn, cc, ch, sc,
                                       B, T, Q, c.st))]
        ps = c.ints('starts', c.rng.integers(0, n + 1), (0, T))
        return [('wn_xent_score_window', (logits, ld, q, ps, plen, rn, cn, cc,
                                          ch, sc, B, T, Q, c.st))]
    if not inplace:
        dlog = c.out('dlogits', (N, Q), ld=ld)
    parts = c.out('loss_partials', lib.wn_xent_partials(N))
    if kind == 'xent':
        return [('wn_xent', (logits, ld, q, dlog, parts, B, T, Q, quirk,
                             c.st))]
    plen = c.ints('lengths', n, (T, 0))
    inv = c.fin('inv_den', 1, kind='pos')
    if kind == 'masked':
        return [('wn_xent_masked', (logits, ld, q, plen, inv, dlog, parts, B,
                                    T, Q, quirk, c.st))]
    ps = c.ints('starts', c.rng.integers(0, n + 1), (0, T))
    return [('wn_xent_window', (logits, ld, q, ps, plen, inv, dlog, parts, B,
                                T, Q, quirk, c.st))]


# a wave per row, four per workgroup, at most 1024 workgroups; Q == 256 takes
# the single-pass path; Q = 123 is refused (Q % 4) before any launch
_XBT = [(1, 1), (5, 333)]


def xent_cases(kind, **kw):
    return [dict(B=B, T=T, Q=Q, kind=kind, **kw) for B, T in _XBT
            for Q in (16, 123, 256)]


def b_softmax64_row(c, Q):
    x = c.fin('logits_row', Q)
    p = c.out('proba', Q)
    return [('wn_softmax64_row', (x, Q, p, c.st))]


# ========================================================== conditioning
def b_gc_bias(c, L, B, ch, G, card, emb=1):
    off_bias, off_gc = 64, 64 + 2 * ch + 32
    blk = off_gc + 2 * G * ch
    stride = blk + 32
    layer = c.fin('layer0', (L, blk), ld=stride)
    pe = c.fin('emb', (card, G)) if emb else None
    ids = c.ints('ids', c.rng.integers(0, card, B), (card - 1, 0)) if emb \
        else None
    out = c.out('out', (L, B, 2 * ch))
    return [('wn_gc_bias', (layer, stride, off_bias, off_gc, G if emb else 0,
                            pe, card if emb else 0, ids, out, L, B, ch,
                            c.st))]


GC_CASES = [dict(L=1, B=1, ch=32, G=4, card=5), dict(L=3, B=3, ch=32, G=4,
                                                     card=5),
            dict(L=2, B=2, ch=64, G=3, card=7),
            dict(L=3, B=1, ch=32, G=4, card=5, emb=0)]


def b_colsum_clip(c, B, T):
    p0, p1 = c.fin('plane0', (B * T, 32)), c.fin('plane1', (B * T, 32))
    part = c.out('part', B * c.lib.wn_colsum_clip_chunks(T) * 64)
    out = c.out('out', (B, 64))
    return [('wn_colsum_clip', (p0, p1, B, T, part, out, c.st))]


# chunks of 512 rows, eight rows per pass of a workgroup
COLSUM_CASES = [dict(B=1, T=1), dict(B=3, T=17), dict(B=3, T=513),
                dict(B=1, T=1025), dict(B=2, T=511)]


def b_gc_grad(c, L, B, ch, G, card):
    off_gc = 64 + 2 * ch + 32
    blk = off_gc + 2 * G * ch
    stride = blk + 32
    layer = c.fin('layer0', (L, blk), ld=stride)
    pe = c.fin('emb', (card, G))
    ids = c.ints('ids', c.rng.integers(0, card, B), (card - 1, 0))
    dsum = c.fin('dsum', (L, B, 2 * ch))
    gl = c.out('glayer0', (L, blk), ld=stride)
    ge = c.out('gemb', (card, G))
    sc = c.out('scratch', L * B * G)
    return [('wn_gc_grad', (layer, stride, off_gc, G, pe, card, ids, dsum, L,
                            B, gl, ge, sc, ch, c.st))]


def _lc_up(c, scales, Lc, use_bias, B, T):
    hop = int(np.prod(scales))
    sp = c.host_array(scales, np.int32)
    m = len(scales)
    n = c.lib.wn_lc_upsample_floats(sp, m, use_bias)
    assert n > 0
    # every row's frame inside F for any offset below hop, which is what both
    # fills of the offsets' bands are
    F = (hop - 1 + T - 1) // hop + 1
    fr = c.fin('frames', (B, F, Lc))
    off = c.ints('off', c.rng.integers(0, hop, B), (hop - 1, 0))
    up = c.fin('up', n, scale=0.5)
    return hop, sp, m, n, F, fr, off, up


def b_lc_upsample_fwd(c, scales, Lc, B, T, use_bias=1, ld=32):
    hop, sp, m, n, F, fr, off, up = _lc_up(c, scales, Lc, use_bias, B, T)
    rows = c.out('rows', (B * T, ld))    # (zeros from column Lc on)
    return [('wn_lc_upsample_fwd', (fr, F, off, up, sp, m, Lc, use_bias, rows,
                                    ld, B, T, c.st))]


def b_lc_upsample_bwd(c, scales, Lc, B, T, use_bias=1, ld=32, ctx=0):
    hop, sp, m, n, F, fr, off, up = _lc_up(c, scales, Lc, use_bias, B, T)
    dr = c.fin('drows', (B * T, Lc), ld=ld)
    ns = c.lib.wn_lc_upsample_bwd_slabs(B * T, n)
    stride = (n + 3) // 4 * 4 + 4
    slabs = c.out('slabs', (ns, n), ld=stride)
    args = (fr, F, off, up, sp, m, Lc, use_bias, dr, ld, B, T, slabs, ns,
            stride)
    if not ctx:
        return [('wn_lc_upsample_bwd', args + (c.st,))]
    df = c.out('dframes', (B, F, Lc))
    dp = c.out('dpart', ns * 2 * Lc)
    return [('wn_lc_upsample_bwd_ctx', args + (df, dp, c.st))]


# four rows per workgroup forward; backward: at least 32 rows per workgroup
LC_UP_CASES = [dict(scales=(4, 5), Lc=12, B=1, T=1),
               dict(scales=(4, 5), Lc=12, B=3, T=33),
               dict(scales=(4, 5), Lc=12, B=2, T=159, use_bias=0),
               dict(scales=(2,), Lc=13, B=3, T=17, ld=16),
               dict(scales=(2, 2, 3), Lc=80, B=1, T=129, ld=80)]


def b_lc_context_fwd(c, p, Lc, Fw, B):
    Fx = Fw + 2 * p + 1
    x = c.fin('x', (B, Fx, Lc))
    w = c.fin('w', ((2 * p + 1) * Lc, Lc), scale=0.2)
    ctx = c.out('ctx', (B, Fw, Lc))
    return [('wn_lc_context_fwd', (x, Fx, w, p, Lc, ctx, Fw, B, c.st))]


def b_lc_context_wgrad(c, p, Lc, Fw, B):
    Fx = Fw + 2 * p + 1
    x = c.fin('x', (B, Fx, Lc))
    d = c.fin('dctx', (B, Fw, Lc))
    n = (2 * p + 1) * Lc * Lc
    ns = c.lib.wn_lc_context_wgrad_slabs(B * Fw, n)
    stride = (n + 3) // 4 * 4 + 4
    slabs = c.out('slabs', (ns, n), ld=stride)
    return [('wn_lc_context_wgrad', (x, Fx, d, Fw, p, Lc, B, slabs, ns,
                                     stride, c.st))]


# four frames per workgroup forward; backward: 32 frames per slab, four rows
# of the [K][Lc] matrix per workgroup
LC_CTX_CASES = [dict(p=0, Lc=1, Fw=1, B=1), dict(p=2, Lc=12, Fw=9, B=2),
                dict(p=8, Lc=13, Fw=33, B=3), dict(p=1, Lc=130, Fw=5, B=1),
                dict(p=2, Lc=12, Fw=65, B=1)]


# ======================================== elementwise, optimizers, exported
_N = (1, 3, 4, 1025)
HYP = dict(adam=(1e-3, 0.9, 0.999, 1e-8), momentum=(0.01, 0.9),
           rmsprop=(1e-3, 0.9, 0.9, 1e-10))


def b_optim(c, rule, n, clip=0, mask=1, ema=1):
    lib = c.lib
    p, g = c.fin('p', n, role='inout'), c.fin('g', n)
    if rule == 'adam':
        state = (c.fin('m', n, role='inout'),
                 c.fin('v', n, role='inout', kind='pos'))
    elif rule == 'momentum':
        state = (c.fin('acc', n, role='inout'),)
    else:
        state = (c.fin('ms', n, role='inout', kind='pos'),
                 c.fin('mom', n, role='inout'))
    pm = c.fin('l2_mask', n, kind='pos') if mask else None
    args = (p, g) + state + (n,) + HYP[rule] + (0.5, 1e-4, pm)
    if not clip:
        return [('wn_' + rule, args + (c.st,))]
    np_ = lib.wn_grad_norm_partials_count()
    parts = c.fin('partials', np_, kind='pos', dtype=F64)
    pe = c.fin('ema', n, role='inout') if ema else None
    no = c.out('norm_out', 1)
    return [('wn_%s_clip' % rule, args + (parts, np_, 0.25, pe, 0.99, no,
                                          c.st))]


def optim_cases(rule, clip):
    return [dict(rule=rule, n=n, clip=clip) for n in _N] + [
        dict(rule=rule, n=1025, clip=clip, mask=0, ema=0)]


def b_grad_norm_partials(c, n):
    g = c.fin('g', n)
    parts = c.out('partials', c.lib.wn_grad_norm_partials_count(), F64)
    return [('wn_grad_norm_partials', (g, n, parts, c.st))]


def b_l2_partials(c, n, mask=1):
    p = c.fin('p', n)
    pm = c.fin('mask', n, kind='pos') if mask else None
    parts = c.out('partials', c.lib.wn_l2_partials_count())
    return [('wn_l2_partials', (p, n, pm, parts, c.st))]


def b_axpy(c, n, mask=1):
    y, x = c.fin('y', n, role='inout'), c.fin('x', n)
    pm = c.fin('mask', n, kind='pos') if mask else None
    return [('wn_axpy', (y, x, 0.5, pm, n, c.st))]


def b_fill(c, n):
    return [('wn_fill', (c.out('p', n), n, 1.5, c.st))]


def b_sum_rows(c, n, rows=3):
    return [('wn_sum_rows', (c.fin('in', (rows, n)), rows, n, c.out('out', n),
                             c.st))]


def b_mu_law_encode(c, n, Q=256):
    thr = np.empty(Q - 1, np.float32)
    assert c.lib.wn_mu_law_thresholds_host(Q, thr.ctypes.data) == 0
    # (the audio becomes codes: both fills of its bands are audio)
    a = c.fin('audio', n, kind='unit', fill=(0.5, -0.5))
    t = c.a.place('thr', thr, F32).data_ptr()
    codes = c.out('codes', n, I32, fill=(Q - 1, 0))
    return [('wn_mu_law_encode', (a, codes, n, t, Q, c.st))]


def b_mu_law_decode(c, n, Q=256):
    lut = np.empty(Q, np.float32)
    assert c.lib.wn_mu_law_decode_table_host(Q, lut.ctypes.data) == 0
    codes = c.codes('codes', n, Q)
    t = c.a.place('lut', lut, F32).data_ptr()
    a = c.out('audio', n)
    return [('wn_mu_law_decode', (codes, a, n, t, Q, c.st))]


def b_time_to_batch(c, n, B=2, C=3, d=2):
    U = (n + d - 1) // d
    x = c.fin('in', (B, n, C))
    y = c.out('out', (B * d, U, C))
    return [('wn_time_to_batch', (x, y, B, n, C, d, c.st))]


def b_batch_to_time(c, n, B=2, C=3, d=2):
    x = c.fin('in', (B * d, n, C))
    y = c.out('out', (B, n * d, C))
    return [('wn_batch_to_time', (x, y, B, n, C, d, c.st))]


def b_causal_conv(c, n, B=2, Cin=5, Cout=7, K=3, d=2):
    x = c.fin('x', (B, n, Cin))
    w = c.fin('w', (K, Cin, Cout))
    y = c.out('y', (B, n, Cout))
    return [('wn_causal_conv', (x, w, y, B, n, Cin, Cout, K, d, c.st))]


# ============================================= corpus gathers, input noise
def _corpus_plan(c, B, step=1, random=0, size=0):
    """Three utterances at odd offsets, four items, two epochs' orders; the
    kernels bounds-check every table entry, and both fills of every table's
    bands are entries in range"""
    lens = np.array([37, 1, 150], np.int32)
    offs = np.array([3, 45, 51], np.int64)
    N = int(offs[-1] + lens[-1]) + 2
    flat = c.fin('flat', N, kind='unit')
    U, P, nE = 3, 4, 2
    uo = c.ints('utt_off', offs, (0, 1), dtype=I64)
    ul = c.ints('utt_len', lens, (1, 0))
    iu = c.ints('item_utt', [0, 1, 2, 2], (U - 1, 0))
    it = c.ints('item_start', [0, 0, 0, 75], (0, 1))
    perm = c.ints('perm', [[2, 0, 3, 1], [1, 3, 0, 2]], (P - 1, 0))
    assert (step * B + B - 1) // P < nE
    plan = (uo, ul, U, iu, it, P, perm, 0, nE, step * B, size, random,
            0x1234567)
    return flat, N, plan, offs, lens


def b_corpus_gather(c, B, T, hist=0, **kw):
    flat, N, plan, _, _ = _corpus_plan(c, B, **kw)
    audio = c.out('audio', (B, T))
    if not hist:
        return [('wn_corpus_gather', (flat, N) + plan + (audio, B, T, c.st))]
    ph, pl = c.out('hist', B, I32), c.out('lens', B, I32)
    return [('wn_corpus_gather_hist', (flat, N) + plan + (hist, audio, ph, pl,
                                                          B, T, c.st))]


def b_corpus_frames(c, B, T, Lc, hop=8, ctx=2, hist=0, frames=1, rows=1,
                    **kw):
    _, _, plan, offs, lens = _corpus_plan(c, B, **kw)
    del c.a.ops['flat']                  # (the frames entries take no audio)
    nfr = (lens + hop - 1) // hop
    fo = np.concatenate([[1], 1 + np.cumsum(nfr)[:-1] + [1, 2]]).astype(np.int64)
    NF = int(fo[-1] + nfr[-1] + 1) * Lc
    fr = c.fin('fr', NF)
    pfo = c.ints('fr_off', fo, (0, 1), dtype=I64)
    pfl = c.ints('fr_len', nfr, (1, 0))
    Fw = int(c.lib.wn_corpus_window_frames(T, hop, ctx))
    pf = c.out('frames', (B, Fw, Lc)) if frames else None
    pr = c.out('rows', (B, T, Lc)) if rows else None
    tail = (hop, ctx, Lc, pf, Fw, pr, B, T, c.st)
    if hist:
        return [('wn_corpus_gather_frames_hist',
                 (fr, NF, pfo, pfl) + plan + (hist,) + tail)]
    return [('wn_corpus_gather_frames', (fr, NF, pfo, pfl) + plan + tail)]


# four samples per thread, a 16-byte load where the source index allows: T at
# remainder 1 and 3 of 4, rows that begin inside a thread's four, a cut to T
# shorter than an item, items shorter than T, a random crop
CORPUS_CASES = [dict(B=3, T=1), dict(B=3, T=33), dict(B=2, T=160),
                dict(B=3, T=75, step=0), dict(B=3, T=20, random=1, size=20),
                dict(B=1, T=150, step=3)]
CORPUS_FR_CASES = [dict(Lc=Lc, **k) for k in CORPUS_CASES for Lc in (5, 12)] + [
    dict(B=3, T=33, Lc=12, rows=0), dict(B=3, T=33, Lc=5, frames=0),
    dict(B=3, T=33, Lc=1, hop=1, ctx=0)]


def b_code_noise(c, B, T, Q=256, fused=0, lengths=1, inplace=0, thresh=1 << 23,
                 width=3):
    keys = c.ints('keys', c.rng.integers(0, 1 << 40, B), (1, 0), dtype=I64)
    n = np.append(c.rng.integers(1, T + 1, B - 1), T)
    pl = c.ints('lengths', n, (T, 0)) if lengths else None
    if fused:
        thr = np.empty(Q - 1, np.float32)
        assert c.lib.wn_mu_law_thresholds_host(Q, thr.ctypes.data) == 0
        # (the audio becomes codes: both fills of its bands are audio)
        a = c.fin('audio', (B, T), kind='unit', fill=(0.5, -0.5))
        t = c.a.place('thr', thr, F32).data_ptr()
        codes = c.out('codes', (B, T), I32, fill=(Q - 1, 0))
        cin = c.out('codes_in', (B, T), I32, fill=(Q - 1, 0))
        return [('wn_mu_law_encode_noisy', (a, codes, cin, keys, pl, B, T, t,
                                            Q, 99, thresh, width, c.st))]
    data = c.rng.integers(0, Q, (B, T))
    if inplace:
        codes = cin = c.ints('codes', data, (Q - 1, 0), role='inout')
    else:
        codes = c.ints('codes', data, (Q - 1, 0))
        cin = c.out('codes_in', (B, T), I32, fill=(Q - 1, 0))
    return [('wn_code_noise', (codes, cin, keys, pl, B, T, Q, 99, thresh,
                               width, c.st))]


# one grid row per clip, four positions per thread, 256 threads: T at
# remainder 1 and 3 of 4 (only clip 0's rows start 16-byte aligned) and past
# one workgroup (1024 positions)
NOISE_CASES = [dict(B=1, T=1), dict(B=3, T=33), dict(B=3, T=160),
               dict(B=2, T=1027, Q=16), dict(B=3, T=35, lengths=0,
                                             thresh=1 << 24)]


def _n(**kw):
    return [dict(n=n, **kw) for n in _N]


ROWS = [
    # ---- GEMMs and reductions
    Row('wn_gemm_nn', b_gemm_nn, NN_CASES, ('A', WN_ERR_MISALIGNED, 4)),
    Row('wn_gemm_nn_split', b_gemm_nn, NN_SPLIT_CASES,
        ('C', WN_ERR_MISALIGNED, 1)),
    Row('wn_gemm_tn', b_gemm_tn, TN_CASES, None),
    Row('wn_gemm_tn_split', b_gemm_tn, TN_SPLIT_CASES,
        ('G', WN_ERR_MISALIGNED, 1)),
    Row('wn_reduce_slabs', b_reduce_slabs, REDUCE_CASES, None),
    Row('wn_reduce_slabs_mt', b_reduce_slabs_mt, MT_CASES,
        ('dst_main', WN_ERR_MISALIGNED, 0)),
    Row('wn_reduce_pair_slabs', b_reduce_pair_slabs, PAIR_CASES,
        ('layer_grad', WN_ERR_MISALIGNED, 0)),
    Row('wn_transpose', b_transpose, TRANSPOSE_CASES, None),
    Row('wn_diag_mfma_peak', b_diag, [dict(blocks=3, iters=2),
                                      dict(blocks=1, iters=-2)], None),
    # ---- layer kernels
    Row('wn_layer_fwd', b_layer_fwd, LAYER_FWD_CASES,
        ('z', WN_ERR_MISALIGNED, 4)),
    Row('wn_layer_bwd2', b_layer_bwd2, LAYER_BWD2_CASES,
        ('dx_out', WN_ERR_MISALIGNED, 1)),
    Row('wn_layer_bwd2_pack', b_layer_bwd2_pack, [dict(L=1), dict(L=7)],
        ('wimg', WN_ERR_MISALIGNED, 1)),
    Row('wn_stack_pack', b_stack_pack, [dict(L=1), dict(L=7, which=1),
                                        dict(L=3, which=2)], None),
    Row('wn_stack_skip_pack', b_stack_skip_pack, [dict(L=1), dict(L=5)], None),
    Row('wn_layer_fwd_k', b_layer_fwd, LAYER_FWD_K_CASES, None),
    Row('wn_layer_bwd_k', b_layer_bwd_k, LAYER_BWD_K_CASES, None),
    Row('wn_layer_wgrad_k', b_layer_wgrad_k, WGRAD_K_CASES, None),
    Row('wn_layer_fwd_blk', b_layer_fwd_blk, BLK_CASES + [
        dict(B=3, T=33, d=2, K=2, CB=2, save_ts=0, bias=0)],
        ('z', WN_ERR_MISALIGNED, 0)),
    Row('wn_layer_bwd_blk', b_layer_bwd_blk, BLK_CASES + [
        dict(B=3, T=33, d=2, K=2, CB=2, dxin=0)],
        ('dx_out', WN_ERR_MISALIGNED, 0)),
    Row('wn_dense_planes', b_dense_planes, DENSE_CASES,
        ('out', WN_ERR_MISALIGNED, 1)),
    Row('wn_dense_planes_gate', b_dense_planes,
        [dict(gate=1, **k) for k in DENSE_CASES if k['C'] > 32],
        ('dag', WN_ERR_MISALIGNED, 1)),
    # ---- causal layer and loss
    Row('wn_causal_gather', b_causal_gather,
        [dict(B=B, T=T, Q=Q, K=K) for (B, T, Q), K in
         zip(_BTQ, (2, 2, 3, 2, 4))], ('x0', WN_ERR_MISALIGNED, 1)),
    Row('wn_causal_wgrad', b_causal_wgrad,
        [dict(B=B, T=T, Q=Q) for B, T, Q in _BTQ], None),
    Row('wn_scalar_causal_fwd', b_scalar_causal_fwd, SCALAR_CASES,
        ('x0', WN_ERR_MISALIGNED, 1)),
    Row('wn_scalar_causal_wgrad', b_scalar_causal_wgrad, SCALAR_CASES, None),
    Row('wn_xent', b_xent, xent_cases('xent') + [
        dict(B=5, T=333, Q=256, kind='xent', inplace=1, quirk=1),
        dict(B=5, T=333, Q=16, kind='xent', inplace=1)],
        ('logits', WN_ERR_MISALIGNED, 5)),
    Row('wn_xent_masked', b_xent, xent_cases('masked') + [
        dict(B=5, T=333, Q=256, kind='masked', inplace=1)],
        ('lengths', 0, 5)),                  # "4-byte aligned"
    Row('wn_xent_window', b_xent, xent_cases('window') + [
        dict(B=5, T=333, Q=16, kind='window', inplace=1, quirk=1)],
        ('starts', 0, 3)),
    Row('wn_xent_score', b_xent, xent_cases('score') + [
        dict(B=5, T=333, Q=256, kind='score', row_nll=0, lengths=0)],
        ('logits', WN_ERR_MISALIGNED, 3)),
    Row('wn_xent_score_window', b_xent, xent_cases('score_window') + [
        dict(B=5, T=333, Q=16, kind='score_window', row_nll=0)],
        ('row_nll', 0, 5)),
    Row('wn_softmax64_row', b_softmax64_row,
        [dict(Q=Q) for Q in (1, 16, 123, 256, 1000)], None),
    # ---- conditioning
    Row('wn_gc_bias', b_gc_bias, GC_CASES, None),
    Row('wn_colsum_clip', b_colsum_clip, COLSUM_CASES, None),
    Row('wn_gc_grad', b_gc_grad, [k for k in GC_CASES if k.get('emb', 1)],
        None),
    Row('wn_lc_upsample_fwd', b_lc_upsample_fwd, LC_UP_CASES, None),
    Row('wn_lc_upsample_bwd', b_lc_upsample_bwd, LC_UP_CASES, None),
    Row('wn_lc_upsample_bwd_ctx', b_lc_upsample_bwd,
        [dict(ctx=1, **k) for k in LC_UP_CASES], None),
    Row('wn_lc_context_fwd', b_lc_context_fwd, LC_CTX_CASES, None),
    Row('wn_lc_context_wgrad', b_lc_context_wgrad, LC_CTX_CASES, None),
    # ---- elementwise and optimizers, n in {1, 3, 4, 1025}
    Row('wn_adam', b_optim, optim_cases('adam', 0), None),
    Row('wn_momentum', b_optim, optim_cases('momentum', 0), None),
    Row('wn_rmsprop', b_optim, optim_cases('rmsprop', 0), None),
    Row('wn_adam_clip', b_optim, optim_cases('adam', 1), None),
    Row('wn_momentum_clip', b_optim, optim_cases('momentum', 1), None),
    Row('wn_rmsprop_clip', b_optim, optim_cases('rmsprop', 1), None),
    Row('wn_grad_norm_partials', b_grad_norm_partials, _n(),
        ('g', WN_ERR_MISALIGNED, 3)),
    Row('wn_l2_partials', b_l2_partials, _n() + [dict(n=1025, mask=0)], None),
    Row('wn_axpy', b_axpy, _n() + [dict(n=1025, mask=0)], None),
    Row('wn_fill', b_fill, _n(), None),
    Row('wn_sum_rows', b_sum_rows, _n() + [dict(n=257, rows=1)], None),
    Row('wn_mu_law_encode', b_mu_law_encode, _n() + [dict(n=1025, Q=16)],
        None),
    Row('wn_mu_law_decode', b_mu_law_decode, _n() + [dict(n=1025, Q=123)],
        None),
    Row('wn_time_to_batch', b_time_to_batch, _n() + [dict(n=23, d=3)], None),
    Row('wn_batch_to_time', b_batch_to_time, _n() + [dict(n=23, d=3)], None),
    Row('wn_causal_conv', b_causal_conv, _n() + [dict(n=37, K=2, d=64)], None),
    # ---- corpus gathers and input noise
    Row('wn_corpus_gather', b_corpus_gather, CORPUS_CASES,
        ('audio', WN_ERR_MISALIGNED, 1)),
    Row('wn_corpus_gather_hist', b_corpus_gather,
        [dict(hist=h, **k) for k in CORPUS_CASES for h in (16, 200)],
        ('lens', 0, 2)),                     # "4-byte aligned"
    Row('wn_corpus_gather_frames', b_corpus_frames, CORPUS_FR_CASES,
        ('rows', WN_ERR_MISALIGNED, 2)),
    Row('wn_corpus_gather_frames_hist', b_corpus_frames,
        [dict(hist=16, **k) for k in CORPUS_FR_CASES],
        ('fr', WN_ERR_MISALIGNED, 2)),
    Row('wn_code_noise', b_code_noise, NOISE_CASES + [
        dict(B=3, T=33, inplace=1)], ('codes', 0, 1)),   # "4-byte aligned"
    Row('wn_mu_law_encode_noisy', b_code_noise,
        [dict(fused=1, **k) for k in NOISE_CASES], ('codes_in', 0, 1)),
]

_STACK = ('needs the private state only the model builds (weight images, '
          'flags, control block, dilations on the device): covered through '
          'views by tests/test_gpu_guard_workspace.py')
_FASTGEN = ('fast-generation family: sizes its own state through its '
            '*_floats / *_bytes / *_words queries, out of scope here')
_HOST = 'writes host memory through a host pointer: no device operand'
EXEMPT = {
    'wn_stack_fwd': _STACK, 'wn_stack_fwd_skip': _STACK,
    'wn_stack_fwd_lc': _STACK, 'wn_stack_bwd': _STACK,
    'wn_stack_bwd_lc': _STACK,
    'wn_stack_bwd_waves': 'a launch-shape query that ' + _HOST,
    'wn_mu_law_thresholds_host': _HOST, 'wn_mu_law_decode_table_host': _HOST,
    'wn_feature_stats': 'has a band test: tests/test_gpu_featnorm.py::'
    'test_stats_match_float64_numpy: NaN behind every clip\'s real frames '
    '(_poisoned), the sums must stay finite; reads only, nothing around acc',
    'wn_feature_normalize': 'has a band test: tests/test_gpu_featnorm.py::'
    'test_normalize_is_the_restated_rule_bit_for_bit (_poisoned input, every '
    'float of a NaN-filled output written) and ::test_normalize_from_a_view_'
    'off_by_four_bytes (the word in front of the output stays NaN)',
    'wn_feature_distance': 'has a band test: tests/test_gpu_synthesis.py::'
    'test_distance_matches_float64_numpy: NaN behind the real frames of both '
    'inputs (_poisoned), the sums must stay finite; reads only',
    'wn_melspec': 'has a band test: tests/test_gpu_features.py::'
    'test_row_stride_and_a_base_off_by_four_bytes: ld = T + 3 with NaN gap '
    'columns and a NaN word in front of the audio, a NaN-filled output',
    'wn_preemphasis': 'has a band test: tests/test_gpu_emphasis.py::'
    'test_pre_leading_dimensions_nan_padding_and_identity: NaN behind the '
    'lengths and in the columns of ld = T + 37, no NaN may come out',
    'wn_deemphasis': 'has a band test: tests/test_gpu_emphasis.py::'
    'test_de_ragged_batch_of_every_length (NaN behind the lengths) and '
    '::test_de_clip_bits_do_not_depend_on_the_batch (clips inside a NaN '
    'batch of ld = T + 3)',
}
EXEMPT.update({'wn_fastgen_' + n: _FASTGEN for n in (
    'init run run_wide step finish persist pre pack batch_init batch_pre '
    'batch_step batch_stages batch_finish batch_step_q batch_finish_q '
    'batch_restart batch_lc_rows lc_bias run_lc run_trunc run_wide_trunc '
    'run_lc_trunc pre_lc step_lc persist_lc batch_pre_lc batch_step_lc '
    'batch_step_lc_q').split()})


def _short(case):
    return ','.join('%s=%s' % (k, ''.join(str(v).split()))
                    for k, v in case.items())


CASES = [pytest.param(r, k, id='%s[%s]' % (r.entry, _short(k)))
         for r in ROWS for k in r.cases]
SKEWED = [pytest.param(r, id='%s[%s+4]' % (r.entry, r.skew[0]))
          for r in ROWS if r.skew]


def _go(lib, row, case, skew=None, code=0):
    c = Ctx(lib, skew)
    calls = row.build(c, **case)
    assert set(n for n, _ in calls) == {row.entry}, calls
    expect = code or c.expect
    if expect:
        # refused before any launch: every band and every operand untouched
        c.a.refill('A')
        got = run_calls(c, calls)
        torch.cuda.synchronize()
        assert got == expect, (row.entry, case, got, expect)
        c.a.check()
        c.a.untouched()
        return
    codes = []
    guard.read_check(c.a, lambda: codes.append(run_calls(c, calls)))
    assert codes == [0, 0], (row.entry, case, codes)


@pytest.mark.parametrize('row,case', CASES)
def test_entry_stays_inside_its_operands(hip_lib, row, case):
    _go(hip_lib, row, case)


@pytest.mark.parametrize('row', SKEWED)
def test_entry_four_bytes_off_alignment(hip_lib, row):
    """skew = (operand, code, case): the operand 4 bytes off its 256-byte
    alignment.  code 0: the entry documents 4-byte alignment for it and must
    pass both checks again; else it must return that code, untouched."""
    name, code, k = row.skew
    _go(hip_lib, row, row.cases[k], skew=name, code=code)


def test_the_checks_see_planted_accesses_on_the_device(hip_lib):
    """The harness itself, on the device, with entries asked for one element
    more than the operand holds (inside the band: nothing else is touched):
    a store one word past the end, a load one row past the end."""
    c = Ctx(hip_lib)
    p = c.out('p', 1025)
    with pytest.raises(guard.GuardError) as e:
        guard.read_check(c.a, lambda: hip_lib.wn_fill(p, 1026, 1.5, c.st))
    assert (e.value.operand, e.value.band, e.value.offset, e.value.count) == \
        ('p', 'back', 1, 1)
    c = Ctx(hip_lib)
    x, y = c.fin('in', (3, 257)), c.out('out', 257)
    with pytest.raises(guard.GuardError) as e:
        guard.read_check(c.a, lambda: hip_lib.wn_sum_rows(x, 4, 257, y, c.st))
    assert (e.value.operand, e.value.band, e.value.offset, e.value.count) == \
        ('out', 'read', 0, 257)
    c = Ctx(hip_lib)
    q = c.codes('codes', 1025, 256)
    lut = c.fin('lut', 256)
    a = c.out('audio', 1026)
    with pytest.raises(guard.GuardError) as e:
        guard.read_check(c.a, lambda: hip_lib.wn_mu_law_decode(q, a, 1026, lut,
                                                               256, c.st))
    assert (e.value.operand, e.value.band, e.value.offset, e.value.count) == \
        ('audio', 'read', 1025, 1)
