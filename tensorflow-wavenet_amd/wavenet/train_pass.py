"""The training pass, host side: what one loss() / predict_proba() call
launches (StepPath, step_path), its launch plans (run_pass) and the eager
forward and backward passes they record -- the counterpart of the reference's
_create_network (model.py:389-442) and of TF autodiff through it.  Functions
take the model first; WaveNetModel._loss and predict_proba call in here."""
import collections

import torch

from . import _lib
from . import local_condition as lcond
from .workspace import CH

# Beside the backward stack of a very small batch (256 - 512 32-row tiles) the
# side stream's TN GEMMs run this fraction of their splits: fewer, longer
# workgroups disturb the stack's dependent chain less (B = 1, T = 16000, 500
# tiles: 1.89 -> 1.80 ms per step at 0.6; 0.75 and 0.4 lose; at B = 2 nothing
# changes; at most one tile per CU is too short for it to matter)
TN_SIDE_SPLIT_FRAC = 0.6

# What one loss() / predict_proba() call launches, decided once per call by
# step_path and the key of its launch plans: the residual stack's
# forward `fwd` ('stack' | 'stack_skip' | 'stack_lc' persistent launches, or
# 'layer' | 'layer_k' | 'blocked' per layer) and backward `bwd` (None, 'stack' |
# 'stack_lc' | 'layer2' | 'layer_k' | 'blocked'), the saved planes `save_ts`
# (0 | 1: tanh + sigmoid | 2: sigmoid), and `pack_both` (the forward's
# wn_stack_pack writes the backward image too), `overlap_tn` (TN GEMMs on the
# side stream), `early_allreduce`, `causal_wgrad`, `gemm_mode`, `variant`.
StepPath = collections.namedtuple('StepPath', [
    'fwd', 'save_ts', 'bwd', 'pack_both', 'overlap_tn', 'early_allreduce',
    'causal_wgrad', 'gemm_mode', 'variant'])


def step_path(net, ws, backward, l2=False):
    """The StepPath of one call on workspace `ws`, from the model's
    switches as they are now and the ones `ws` froze (stack_bwd, the
    variant word).  l2: L2 regularisation is on (it adds to the whole
    bucket after the backward pass: the tail all-reduce must wait)."""
    layers, lc = net._layer_path(), '_lc' if net.Lc else ''
    fwd = layers
    if net.stack_fwd and net._stack_ok():
        # (small batches: the skip sum inside the stack launch)
        skip = (net.stack_fwd_skip and net.gemm_mode == 'fp32' and
                not net.residual_postproc and ws.fwd_skip_ok)
        fwd = 'stack_skip' if skip else 'stack' + lc
    if not backward:
        return StepPath(fwd, 0, None, False, False, False, None,
                        net.gemm_mode, ws.stack_variant)
    bwd = layers
    if layers == 'layer':
        bwd = 'stack' + lc if net._stack_bwd_ok() and ws.stack_bwd \
            else 'layer2'
    if net.Lc and bwd != 'stack_lc':
        # (a training workspace reserved while stack_bwd was off)
        raise NotImplementedError(net.LC_SUPPORTED)
    from . import parallel
    early = bool(net.dp_overlap_allreduce and not l2 and
                 parallel.is_distributed())
    causal = (None if layers == 'blocked' else 'scalar' if net.scalar_input
              else 'segsum' if net.KW == 2 and net.Q <= 256 else 'onehot')
    return StepPath(fwd, 2 if layers == 'layer' else 1, bwd,
                    fwd.startswith('stack') and bwd.startswith('stack'),
                    net._overlap_tn_on(ws), early, causal,
                    net.gemm_mode, ws.stack_variant)


def early_allreduce(net):
    from . import parallel
    _lib.call_py(lambda: parallel.begin_tail_allreduce(net))


def side_stream(net):
    if getattr(net, '_side', None) is None:
        # lower priority than the default stream: the residual-stack
        # kernels on the main stream are the critical path
        net._side = torch.cuda.Stream(device=net.device, priority=0)
    return net._side


def bias_fg(net, ws_bias, ids, B):
    """Per-(layer, clip) filter|gate bias (+ GC 1x1 conv of the broadcast
    embedding, model.py:272-290).  Returns (tensor or None, clip stride)."""
    if not net.use_biases and ids is None:
        return None, 0
    nb = B if ids is not None else 1
    W2 = 2 * net.CHn                  # filter | gate, padded channels
    out = ws_bias.view(-1)[:net.L * nb * W2].view(net.L, nb, W2)
    emb = net._seg(net.params, 'emb') if ids is not None else None
    _lib.call('wn_gc_bias', _lib.ptr(net._layer_block(net.params, 0)),
              net.layer_stride, net.OFF_BF, net.OFF_GC, net.G or 0,
              _lib.ptr(emb), net.card or 0, _lib.ptr(ids), _lib.ptr(out),
              net.L, nb, net.CHn, _lib.stream())
    return out, (W2 if ids is not None else 0)


def nn_seq(net, calls):
    """A sequence of row-wise dependent wn_gemm_nn calls (argument tuples
    without the stream), one launch each.  (Round 4 also ran them as ONE
    persistent launch with row-block dependencies inside: bitwise equal,
    worth at most 0.4 % of a B = 8 step and a loss at small batches;
    removed in round 5, DESIGN.md.)"""
    st = _lib.stream()
    for c in calls:
        nn(net, *(c + (st,)))


def nn(net, *args):
    """wn_gemm_nn (or, when `gemm_mode` asks for it, wn_gemm_nn_split),
    optionally bracketed by HIP events on the launch stream (bench.py's
    live roofline measurement)."""
    name = 'wn_gemm_nn'
    if net.gemm_mode != 'fp32':
        nprod = {'bf16x3': 3, 'bf16x6': 6, 'bf16x9': 9}[net.gemm_mode]
        M, N, K = args[-5], args[-4], args[-3]
        if K % 16 == 0:
            # one scratch buffer per WEIGHT (its address), not per shape:
            # equal-shaped GEMMs never share pieces
            key = (args[4], K, N)
            buf = net._wsplit.get(key)
            if buf is None:
                nb = _lib.load().wn_gemm_split_w_bytes(K, N)
                buf = torch.empty(nb // 4, dtype=torch.int32,
                                  device=net.device)
                net._wsplit[key] = buf
            name = 'wn_gemm_nn_split'
            args = args[:-1] + (_lib.ptr(buf), nprod, args[-1])
    k = -7 if name == 'wn_gemm_nn_split' else -5
    _lib.call_timed(name, args, 2.0 * args[k] * args[k + 1] * args[k + 2],
                    net._gemm_events)


def stage_ids(net, ws, ids):
    """GC ids into a workspace-owned buffer, so that recorded launch
    arguments never point at a caller's temporary."""
    if ids is None:
        return None
    if ids.data_ptr() != ws.gc_ids.data_ptr():
        ws.gc_ids.copy_(ids)
    return ws.gc_ids


def stage_codes(ws, q, q_in=None):
    """Codes into the workspace: q [B, T] into ws.q, which the network reads
    and the loss labels with -- or, where the inputs differ from the targets
    (q_in given), q_in into ws.q and the clean q into ws.q_tgt.  Returns the
    buffer the cross-entropy / scoring launch gets as its `q`.  (Codes that
    were written into these buffers in the first place are not copied.)"""
    if q_in is None:
        ws.q.copy_(q.reshape(-1))
        return ws.q
    if q_in.data_ptr() != ws.q.data_ptr():
        ws.q.copy_(q_in.reshape(-1))
    if q.data_ptr() != ws.q_tgt.data_ptr():
        ws.q_tgt.copy_(q.reshape(-1))
    return ws.q_tgt


def run_pass(net, tag, ws, ids, path):
    """The forward ('fwd') or backward ('bwd') pass through a recorded
    launch plan (see _lib.record), keyed by the call's StepPath."""
    eager = forward_eager if tag == 'fwd' else backward_eager
    ids = stage_ids(net, ws, ids)
    if not net.use_launch_plans or (tag == 'bwd' and path.bwd == 'blocked'):
        # (the channel-block backward's gradient-block copies are torch
        # ops a launch plan cannot replay)
        return eager(net, ws, ids, path)
    key = (tag, path, ids is not None, _lib.stream(),
           net.params.data_ptr(), net.grads.data_ptr())
    plan = ws.plans.get(key, 0)
    if plan == 0:                 # first use of this workspace: eager
        ws.plans[key] = None
        eager(net, ws, ids, path)
    elif plan is None:            # second use: record while executing
        with _lib.record() as rec:
            eager(net, ws, ids, path)
        ws.plans[key] = rec.plan
    else:
        _lib.replay(plan, net._gemm_events)


# ------------------------------------------------------------------ forward
def forward_eager(net, ws, ids, path):
    """_create_network (model.py:389-442) on codes ws.q -> ws.logits."""
    st = _lib.stream()
    B, T, N, L, S, Q = ws.B, ws.T, ws.N, net.L, net.S, net.Q
    P = net.params
    wc = net._seg(P, 'causal')
    for cb in range(net.CB):              # one plane per channel block
        if net.scalar_input:
            _lib.call('wn_scalar_causal_fwd', _lib.ptr(ws.audio),
                      _lib.ptr(wc[cb * CH:]), net.CHn, _lib.ptr(ws.X[cb]),
                      B, T, net.initial_filter_width, st)
        else:
            _lib.call('wn_causal_gather', _lib.ptr(ws.q),
                      _lib.ptr(wc[cb * CH:]), _lib.ptr(ws.X[cb]), B, T, Q,
                      net.KW, net.CHn, st)
    bias, bstride = bias_fg(net, ws.bias_fg, ids, B)
    save_ts = path.save_ts
    if path.fwd == 'blocked':
        from . import blocked
        blocked.forward_layers(net, ws, bias, bstride, bool(save_ts), st)
    elif path.fwd.startswith('stack'):
        fwd_stack(net, ws, path, bias, bstride, st)
    else:                      # 'layer' / 'layer_k': one launch per layer
        for l, d in enumerate(net.dilations):
            last = l == L - 1
            fargs = (_lib.ptr(ws.X[l]),
                     None if last else _lib.ptr(ws.X[l + 1]),
                     _lib.ptr(ws.Z[l]),
                     _lib.ptr(ws.TH[l]) if save_ts == 1 else None,
                     _lib.ptr(ws.SG[l]) if save_ts else None,
                     _lib.ptr(net._layer_block(P, l)),
                     None if bias is None else _lib.ptr(bias[l]), bstride,
                     B, T, int(d))
            if path.fwd == 'layer_k':
                _lib.call('wn_layer_fwd_k', *fargs, net.KW,
                          0 if last else 1, 1 if save_ts else 0, st)
            else:
                _lib.call('wn_layer_fwd', *fargs, 0 if last else 1,
                          int(save_ts), st)
    fuse_skip = path.fwd == 'stack_skip'
    bsum = None
    if net.use_biases and not fuse_skip:
        _lib.call('wn_sum_rows', _lib.ptr(net._seg(P, 'skip_b')), L, S,
                  _lib.ptr(ws.bsum), st)
        bsum = ws.bsum
    # total = sum_l z_l * Ws_l (+ sum_l bs_l); h1 = relu(total)
    LP, C = L * net.CB, net.CHn      # planes, padded channels
    b1 = net._seg(P, 'post1_b') if net.use_biases else None
    b2 = net._seg(P, 'post2_b') if net.use_biases else None
    rp = net.residual_postproc
    skip_gemm = [] if fuse_skip else [
        (_lib.ptr(ws.Z), 0, LP, N * CH,
         _lib.ptr(net._seg(P, 'skip_w')), S, _lib.ptr(bsum), None, 0,
         None, 0, _lib.ptr(ws.h1), S, 0, 0,
         _lib.ptr(ws.total) if net.residual_postproc else None,
         N, S, L * C, 1)]
    nn_seq(net, skip_gemm + [
        (_lib.ptr(ws.h1), S, 0, 0,
         _lib.ptr(net._seg(P, 'post1_w')), S, _lib.ptr(b1), None, 0,
         _lib.ptr(ws.total) if rp else None, S, _lib.ptr(ws.h2), S, 0,
         0, _lib.ptr(ws.c1) if (rp and ws.training) else None,
         N, S, S, 1),
        (_lib.ptr(ws.h2), S, 0, 0,
         _lib.ptr(net._seg(P, 'post2_w')), Q, _lib.ptr(b2), None, 0,
         None, 0, _lib.ptr(ws.logits), Q, 0, 0, None, N, Q, S, 0)])


def fwd_stack(net, ws, path, bias, bstride, st):
    """All L layers in one persistent launch (csrc/wn_stack.hip) behind
    their transposed weight images (wn_stack_pack, one small launch)."""
    B, T, N, L, S = ws.B, ws.T, ws.N, net.L, net.S
    P = net.params
    _lib.call('wn_stack_pack', _lib.ptr(net._layer_block(P, 0)),
              net.layer_stride, _lib.ptr(ws.wimg_f),
              _lib.ptr(ws.wimg_b) if path.pack_both else None, L, st)
    save = path.save_ts != 0
    stack_args = (_lib.ptr(ws.X), _lib.ptr(ws.Z),
                  _lib.ptr(ws.SG) if save else None,
                  _lib.ptr(ws.wimg_f),
                  None if bias is None else _lib.ptr(bias),
                  0 if bias is None else bias.shape[1] * bias.shape[2],
                  bstride, _lib.ptr(net._dil_dev),
                  _lib.ptr(ws.stack_flags), _lib.ptr(ws.stack_ctl),
                  _lib.ptr(ws.loss_parts),
                  L, B, T, 1 if save else 0, ws.stack_variant)
    # (flops 0: timed in bench.py's instrumented pass for its HBM roofline)
    if path.fwd == 'stack_skip':
        # small batches: the skip sum h1 = relu(sum_l z_l Ws_l + sum_l bs_l)
        # inside the stack launch (wn_stack_fwd_skip: a partner wave per
        # tile; the launch's matrix pipe is three quarters idle otherwise)
        if getattr(ws, 'skimg', None) is None:
            ws.skimg = torch.empty(
                int(_lib.load().wn_stack_skip_img_floats(L)),
                dtype=torch.float32, device=net.device)
        bsum_f = None
        if net.use_biases:
            _lib.call('wn_sum_rows', _lib.ptr(net._seg(P, 'skip_b')), L,
                      S, _lib.ptr(ws.bsum), st)
            bsum_f = ws.bsum
        _lib.call('wn_stack_skip_pack', _lib.ptr(net._seg(P, 'skip_w')),
                  L, _lib.ptr(ws.skimg), st)
        _lib.call_timed('wn_stack_fwd_skip', stack_args + (
            _lib.ptr(ws.skimg), _lib.ptr(bsum_f), _lib.ptr(ws.h1), st),
            0.0, net._gemm_events)
    elif path.fwd == 'stack_lc':
        # local conditioning: the per-row filter | gate addends of all
        # layers, lc [N][Lcp] x lc_w [Lcp][L * 64], then the stack
        # launch that adds them (32-row tiles: the workspace's variant)
        W64 = L * 64
        _lib.call_timed('wn_gemm_nn', (
            _lib.ptr(ws.lc), net.Lcp, 0, 0,
            _lib.ptr(net._seg(P, 'lc_w')), W64, None, None, 0, None,
            0, _lib.ptr(ws.lc_add), W64, 0, 0, None, N, W64, net.Lcp,
            0, st), 2.0 * N * W64 * net.Lcp, net._gemm_events)
        _lib.call_timed('wn_stack_fwd_lc', stack_args + (
            _lib.ptr(ws.lc_add), W64, st), 0.0, net._gemm_events)
    else:
        _lib.call_timed('wn_stack_fwd', stack_args + (st,), 0.0,
                        net._gemm_events)


# ------------------------------------------------------------------ backward
def backward_eager(net, ws, ids, path):
    """Hand-written gradient of loss() (the reference uses TF autodiff of
    model.py:628-685).  Consumes ws.logits == dlogits (in place)."""
    st = _lib.stream()
    bwd_post(net, ws, path, st)
    if path.bwd == 'blocked':
        # channel-block path: residual stack, causal layer and global
        # conditioning gradients (wavenet/blocked.py)
        from . import blocked
        if path.overlap_tn:
            main_s = torch.cuda.current_stream()
            _lib.call_py(lambda: main_s.wait_event(ws.ev_join))
        blocked.backward_layers(net, ws, ids, st)
        return
    # residual stack, last layer first, down to dL/dx_0
    run = {'layer2': bwd_layer2,
           'layer_k': bwd_layer_k}.get(path.bwd, bwd_stack)
    backward_tail(net, ws, ids, path, run(net, ws, path, st))


def bwd_post(net, ws, path, st):
    """The data gradients first -- dc1 = (dlogits W2^T) * [c1 > 0],
    dtotal = (dc1 W1^T) * [total > 0] (+ dh2 when residual_postproc),
    dZ planes = dtotal Ws_all^T -- as ONE chained launch (a 128-row block
    of a GEMM starts when that row block of the previous one is stored),
    then the three weight-gradient (TN) GEMMs, whose operands all exist
    by then: dW2 = h2^T dlogits, dW1 = h1^T dc1, dWs_all = Z^T dtotal
    (+ column sums = the bias gradients)."""
    N, L, S, Q = ws.N, net.L, net.S, net.Q
    P, Gr = net.params, net.grads
    rp = net.residual_postproc
    dlog = ws.logits
    LP, C = L * net.CB, net.CHn      # planes, padded channels
    _lib.call('wn_transpose', _lib.ptr(net._seg(P, 'post2_w')), S, Q, Q,
              _lib.ptr(ws.w2t), S, st)
    _lib.call('wn_transpose', _lib.ptr(net._seg(P, 'post1_w')), S, S, S,
              _lib.ptr(ws.w1t), S, st)
    _lib.call('wn_transpose', _lib.ptr(net._seg(P, 'skip_w')), L * C, S,
              S, _lib.ptr(ws.wst), L * C, st)
    nn_dc1 = (_lib.ptr(dlog), Q, 0, 0, _lib.ptr(ws.w2t), S,
              None, _lib.ptr(ws.c1 if rp else ws.h2), S, None, 0,
              _lib.ptr(ws.dc1), S, 0, 0, _lib.ptr(ws.dh2) if rp else None,
              N, S, Q, 0)
    nn_dtotal = (_lib.ptr(ws.dc1), S, 0, 0, _lib.ptr(ws.w1t), S,
                 None, _lib.ptr(ws.h1), S, _lib.ptr(ws.dh2) if rp else None,
                 S, _lib.ptr(ws.dtotal), S, 0, 0, None, N, S, S, 0)
    nn_dz = (_lib.ptr(ws.dtotal), S, 0, 0, _lib.ptr(ws.wst),
             L * C, None, None, 0, None, 0, _lib.ptr(ws.dZ), 0, LP,
             N * CH, None, N, L * C, S, 0)
    tns = [('post2', _lib.ptr(ws.h2), S, 0, 0, _lib.ptr(dlog), Q, S, Q,
            _lib.ptr(net._seg(Gr, 'post2_w')),
            _lib.ptr(net._seg(Gr, 'post2_b'))),
           ('post1', _lib.ptr(ws.h1), S, 0, 0, _lib.ptr(ws.dc1), S, S, S,
            _lib.ptr(net._seg(Gr, 'post1_w')),
            _lib.ptr(net._seg(Gr, 'post1_b'))),
           # skip convs: dbs_l = colsum(dtotal) for every l
           ('skip', _lib.ptr(ws.Z), 0, LP, N * CH, _lib.ptr(ws.dtotal), S,
            L * C, S, _lib.ptr(net._seg(Gr, 'skip_w')),
            _lib.ptr(net._seg(Gr, 'skip_b')), L, S)]
    if not path.overlap_tn:
        nn_seq(net, [nn_dc1, nn_dtotal, nn_dz])
        for key, *a in tns:
            tn(net, ws, path, st, ws.region[key], *a)
        if path.early_allreduce:
            # skip / post-processing gradients are complete on this stream:
            # their all-reduce runs beside the backward stack
            early_allreduce(net)
        return
    # small batches: the TN GEMMs run on a side stream beside the dZ GEMM
    # and the backward stack, so the dZ GEMM stays a launch of its own
    # behind the fork.  The fork: everything the three TN GEMMs read
    # exists now (forking behind the dZ GEMM instead, or another order of
    # the three, changes nothing at B = 1: 1.80 ms either way)
    nn_seq(net, [nn_dc1, nn_dtotal])
    main_s = torch.cuda.current_stream()
    side_s = side_stream(net)
    _lib.call_py(lambda: (ws.ev_fork.record(main_s),
                          side_s.wait_event(ws.ev_fork)))
    for key, *a in tns:
        tn(net, ws, path, side_s.cuda_stream, ws.region[key + '_side'], *a)
    _lib.call_py(lambda: ws.ev_join.record(side_s))
    nn(net, *(nn_dz + (st,)))


def reduce_slabs(reg, dst, st, count=None, offset=0, n=None, replicate=1,
                 rep_stride=0):
    """dst[0:n] = the fixed-order sum over the slabs of region `reg` (a
    workspace.SlabRegion; count: the slabs this call's producer wrote, where
    fewer than allocated).  offset, n: floats [offset, offset + n) of every
    slab instead of its first reg.n; replicate: copies of the sum,
    rep_stride floats apart."""
    _lib.call('wn_reduce_slabs', _lib.ptr(reg.buf),
              reg.count if count is None else count, reg.stride, 1, 0, offset,
              reg.n if n is None else n, dst, 0, replicate, rep_stride, st)


def tn(net, ws, path, st, reg, A, lda, a_planes, a_pstride, Gm, ldg, mw, nw,
       dst, dst_bias, replicate=1, rep_stride=0):
    """dst = A^T Gm (+ its column sums into dst_bias): one wn_gemm_tn into
    the per-split slabs of region `reg` on stream `st`, then their
    fixed-order sum."""
    lib = _lib.load()
    N = ws.N
    ub = 1 if net.use_biases else 0
    sp, sl = reg.count, reg.stride
    if path.overlap_tn and 256 < ws.B * ((ws.T + 31) // 32) <= 512:
        sp = max(1, int(sp * TN_SIDE_SPLIT_FRAC))
    # the slabs' matrix and column sums go through ONE reduction launch
    # when the shapes allow; then the column sums are "spread" too:
    # every tile row of a split sums its share (wn_gemm_tn,
    # want_colsum = 2)
    mt = bool(ub and dst_bias is not None and (mw * nw) % 4 == 0 and
              nw % 4 == 0 and sl % 4 == 0 and rep_stride % 4 == 0)
    tr = int(lib.wn_gemm_tn_tail_rows(mw, nw)) \
        if mt and path.gemm_mode == 'fp32' else 1
    if path.gemm_mode != 'fp32' and N % 16 == 0:
        # opt-in split-bf16 products (fewer, larger splits)
        sp = min(sp, lib.wn_gemm_tn_splits(N, mw, nw, 2))
        _lib.call('wn_gemm_tn_split', A, lda, a_planes, a_pstride, Gm,
                  ldg, _lib.ptr(reg.buf), sp, N, mw, nw, ub,
                  int(path.gemm_mode[-1]), st)
    else:
        _lib.call_timed('wn_gemm_tn',
                        (A, lda, a_planes, a_pstride, None, 0, ws.T,
                         Gm, ldg, _lib.ptr(reg.buf), sp, N, mw, nw,
                         2 if tr > 1 else ub,
                         st), 2.0 * N * mw * nw, net._gemm_events)
    if mt:
        # matrix and column sums (bias gradient) in one launch
        _lib.call('wn_reduce_slabs_mt', _lib.ptr(reg.buf), sp, sl,
                  mw * nw, dst, nw, dst_bias, replicate, rep_stride,
                  tr, st)
        return
    reduce_slabs(reg, dst, st, sp)
    if ub and dst_bias is not None:
        reduce_slabs(reg, dst_bias, st, sp, offset=mw * nw, n=nw,
                     replicate=replicate, rep_stride=rep_stride)


def bwd_stack(net, ws, path, st):
    """All L layers in one persistent launch (csrc/wn_stack.hip)."""
    B, T, L = ws.B, ws.T, net.L
    tsum = None if ws.dsum is None else \
        ws.tilesum16 if ws.stack_rows == 16 else ws.tilesum
    if not path.pack_both:
        _lib.call('wn_stack_pack', _lib.ptr(net._layer_block(net.params, 0)),
                  net.layer_stride, None, _lib.ptr(ws.wimg_b), L, st)
    bargs = (
        _lib.ptr(ws.X), _lib.ptr(ws.Z),
        _lib.ptr(ws.SG), _lib.ptr(ws.dZ), _lib.ptr(ws.DX),
        ws.N * CH if ws.keep_dx else 0,
        _lib.ptr(ws.DQ), _lib.ptr(ws.wimg_b), _lib.ptr(ws.lslabs),
        ws.lslabs.shape[1] * net.LAYER_BLOCK,
        None if tsum is None else _lib.ptr(tsum),
        _lib.ptr(net._dil_dev), _lib.ptr(ws.stack_flags_b),
        _lib.ptr(ws.stack_ctl_b),
        _lib.ptr(ws.loss_parts[1:]), L, B, T, ws.stack_variant)
    if path.bwd == 'stack_lc':
        # ... that also stores da_f | da_g of every row and layer
        _lib.call_timed('wn_stack_bwd_lc', bargs + (
            _lib.ptr(ws.lc_da), L * 64, st), 0.0, net._gemm_events)
    else:
        _lib.call_timed('wn_stack_bwd', bargs + (st,), 0.0,
                        net._gemm_events)
    return ws.DX[0]


def bwd_layer2(net, ws, path, st):
    """One wn_layer_bwd2 launch per layer, chained through dx only."""
    B, T, L, P = ws.B, ws.T, net.L, net.params
    tsum = None if ws.dsum is None else ws.tilesum
    # transposed weight images of all layers (the kernels DMA them
    # into LDS): one small launch per step
    _lib.call('wn_layer_bwd2_pack', _lib.ptr(net._layer_block(P, 0)),
              net.layer_stride, _lib.ptr(ws.wimg), L, st)
    dxin, xp = None, 0
    for l in range(L - 1, -1, -1):
        dxo = ws.dx[xp]
        _lib.call('wn_layer_bwd2', _lib.ptr(ws.X[l]), _lib.ptr(ws.Z[l]),
                  _lib.ptr(ws.SG[l]), _lib.ptr(ws.dZ[l]),
                  _lib.ptr(dxin), _lib.ptr(dxo),
                  _lib.ptr(net._layer_block(P, l)),
                  _lib.ptr(ws.wimg[l]), _lib.ptr(ws.lslabs[l]),
                  None if tsum is None else _lib.ptr(tsum[l]),
                  B, T, int(net.dilations[l]), st)
        dxin, xp = dxo, 1 - xp
    return dxin


def bwd_layer_k(net, ws, path, st):
    """Generic filter width (wn_layer_*_k; also a K = 2 model with
    `generic_layers` forced, tests): phase A of layer l - 1 and phase B
    of layer l per launch, pre-activation gradients through two ping-pong
    plane pairs, weight gradients per layer into slabs."""
    B, T, L, P = ws.B, ws.T, net.L, net.params

    def da(p):
        return ws.da[p][0], ws.da[p][1]

    def layer_bwd(*a):           # (..., B, T, d, do_b, do_a, stream)
        _lib.call('wn_layer_bwd_k', *a[:14], net.KW, *a[14:16], 1, 0, a[16])

    def layer_wgrad(*a):         # (..., nslab, B, T, d, stream)
        _lib.call('wn_layer_wgrad_k', *a[:10], net.KW, 0, net.KW, 1, 0, a[10])
    cur = 0
    f, g = da(cur)
    # phase A of the last layer (no gradient flows into its x' output)
    layer_bwd(None, None, None, None, None,
              _lib.ptr(ws.dZ[L - 1]), _lib.ptr(ws.TH[L - 1]),
              _lib.ptr(ws.SG[L - 1]),
              _lib.ptr(net._layer_block(P, L - 1)), _lib.ptr(f),
              _lib.ptr(g), B, T, 1, 0, 1, st)
    dxin, xp = None, 0    # dL/dx' of layer l (None for the last layer)
    for l in range(L - 1, -1, -1):
        d = int(net.dilations[l])
        f, g = da(cur)
        dxo = ws.dx[xp]
        layer_wgrad(_lib.ptr(ws.X[l]), _lib.ptr(f), _lib.ptr(g),
                    None if dxin is None else _lib.ptr(ws.Z[l]),
                    None if dxin is None else _lib.ptr(dxin),
                    _lib.ptr(ws.lslabs[l]), ws.region['layers_k'].count, B, T,
                    d, st)
        if ws.dsum is not None:
            _lib.call('wn_colsum_clip', _lib.ptr(f), _lib.ptr(g), B, T,
                      _lib.ptr(ws.dsum_part), _lib.ptr(ws.dsum[l]), st)
        if l > 0:
            fn, gn = da(1 - cur)
            layer_bwd(_lib.ptr(f), _lib.ptr(g),
                      None if dxin is None else _lib.ptr(dxin),
                      _lib.ptr(dxo), _lib.ptr(net._layer_block(P, l)),
                      _lib.ptr(ws.dZ[l - 1]), _lib.ptr(ws.TH[l - 1]),
                      _lib.ptr(ws.SG[l - 1]),
                      _lib.ptr(net._layer_block(P, l - 1)), _lib.ptr(fn),
                      _lib.ptr(gn), B, T, d, 1, 1, st)
            cur = 1 - cur
        else:
            layer_bwd(_lib.ptr(f), _lib.ptr(g),
                      None if dxin is None else _lib.ptr(dxin),
                      _lib.ptr(dxo), _lib.ptr(net._layer_block(P, l)),
                      None, None, None, None, None, None, B, T, d, 1, 0,
                      st)
        dxin, xp = dxo, 1 - xp
    return dxin


def backward_tail(net, ws, ids, path, dxin):
    """After the residual stack: slab reductions of the layer-block
    gradients, causal-layer and global-conditioning gradients."""
    if path.overlap_tn:
        main_s = torch.cuda.current_stream()
        _lib.call_py(lambda: main_s.wait_event(ws.ev_join))     # join
        if path.early_allreduce:
            # (small batches: the side stream's weight-gradient GEMMs have
            # just joined; the tail's all-reduce runs beside the slab
            # reductions and the causal / conditioning gradients)
            early_allreduce(net)
    st = _lib.stream()
    B, T, N, L, Q = ws.B, ws.T, ws.N, net.L, net.Q
    P, Gr = net.params, net.grads
    stack = path.bwd.startswith('stack')
    if path.bwd != 'layer_k' and ws.dsum is not None:
        # per-clip sums of da_l for every layer from the per-tile sums the
        # fused kernel wrote (fixed order over a clip's tiles)
        tile_rows = ws.stack_rows if stack else 32
        tpc = (T + tile_rows - 1) // tile_rows
        _lib.call('wn_reduce_slabs', _lib.ptr(ws.tilesum), tpc, 64, L * B,
                  tpc * 64, 0, 64, _lib.ptr(ws.dsum), 64, 1, 0, st)
    # layer-block gradients: fixed-order sum of the per-workgroup slabs the
    # backward that ran wrote, a batch of L layers
    reg = ws.region['layers_stack' if stack else
                    'layers_2' if path.bwd == 'layer2' else 'layers_k']
    lo, _ = net.segments['layers']
    _lib.call('wn_reduce_slabs', _lib.ptr(reg.buf), reg.count, reg.stride, L,
              ws.lslabs.shape[1] * reg.stride, 0, reg.n, _lib.ptr(Gr[lo:]),
              net.layer_stride, 1, 0, st)
    # causal layer: dWc[1][v] = sum_t [q[t]==v] dx0[t]; dWc[0][v] likewise
    # with q[t-1]
    gc_ = net._seg(Gr, 'causal')
    if path.causal_wgrad == 'scalar':
        reg = ws.region['causal_scalar']
        _lib.call('wn_scalar_causal_wgrad', _lib.ptr(ws.audio),
                  _lib.ptr(dxin), _lib.ptr(reg.buf), reg.count, B, T,
                  net.initial_filter_width, st)
        reduce_slabs(reg, _lib.ptr(gc_), st)
    elif path.causal_wgrad == 'segsum':
        reg = ws.region['causal_segsum']
        _lib.call('wn_causal_wgrad', _lib.ptr(ws.q), _lib.ptr(dxin),
                  _lib.ptr(reg.buf), reg.count, B, T, Q, st)
        reduce_slabs(reg, _lib.ptr(gc_), st)
    else:
        # (one-hot operand generated on the fly)
        K, reg = net.KW, ws.region['causal_onehot']
        for tap in range(K):
            shift = (K - 1 - tap) + (K - 1) // 2
            _lib.call('wn_gemm_tn', None, 0, 0, 0, _lib.ptr(ws.q), shift,
                      T, _lib.ptr(dxin), CH, _lib.ptr(reg.buf), reg.count, N,
                      Q, CH, 0, st)
            reduce_slabs(reg, _lib.ptr(gc_[tap * Q * CH:]), st)
    if net.Lc:
        lcond.backward(net, ws, st)
    if ws.dsum is not None:
        _lib.call('wn_gc_grad', _lib.ptr(net._layer_block(P, 0)),
                  net.layer_stride, net.OFF_GC, net.G,
                  _lib.ptr(net._seg(P, 'emb')), net.card, _lib.ptr(ids),
                  _lib.ptr(ws.dsum), L, B,
                  _lib.ptr(net._layer_block(Gr, 0)),
                  _lib.ptr(net._seg(Gr, 'emb')), _lib.ptr(ws.gc_part),
                  net.CHn, st)
