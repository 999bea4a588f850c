"""The training / forward workspace: caller-owned device buffers for one
(B, T) shape, the slab regions weight-gradient producers write into, and the
model's cache of workspaces (`get`).  Functions take the model first."""
import collections

import numpy as np
import torch

from . import _lib
from . import local_condition as lcond

CH = 32                      # channels per activation plane (one block)

# One region of per-workgroup (or per-split) partial results that a producer
# writes and wn_reduce_slabs sums in a fixed order.  buf: the tensor the
# producer writes; count: slabs written (the allocated maximum: a call may
# use fewer); stride: floats between slabs; n: floats of each slab summed
SlabRegion = collections.namedtuple('SlabRegion', 'buf count stride n')


class _Workspace(object):
    """Caller-owned device buffers for one (B, T) shape (the library never
    allocates).  Sized for 288 GB HBM: everything stays resident.  A workspace
    for a smaller T (same B) is carved out of an existing larger one
    (`parent`) without allocating -- the windowed naive generation path calls
    predict_proba with a growing T."""

    def __init__(self, net, B, T, training, parent=None):
        dev = net.device
        L, S, Q = net.L, net.S, net.Q
        CB, CHn = net.CB, net.CHn       # channel blocks, padded channels
        LP = L * CB                     # activation planes per tensor
        N = B * T
        self.B, self.T, self.N, self.training = B, T, N, training
        # (the variant word of the stack launches is fixed per workspace, and so
        # is the library's answer whether wn_stack_fwd_skip covers the shape)
        self.stack_variant = net._stack_variant_for_launch()
        self.capacity = N if parent is None else parent.capacity
        lib = _lib.load()
        self.fwd_skip_ok = bool(lib.wn_stack_fwd_skip_ok(B, T, S,
                                                         self.stack_variant))

        # INVARIANT, "a view fits its owner": every buffer a view (`parent`
        # given: same B, shorter T, same model switches) asks for here has at
        # most as many elements as the owner's buffer of that name, so the
        # reinterpretation below never runs past the owner's memory.  It holds
        # because each size is either independent of T or non-decreasing in
        # it -- except the slab count of wn_stack_bwd, for which the owner
        # asks the library about every shorter shape (_view_stack_slabs).
        # Guard: the sweep of tests/test_workspace_host.py over model kinds,
        # variant words, B and T; a new size that can shrink as T grows must
        # be bounded the same way, never allocated per view.
        def alloc(name, shape, dtype=torch.float32, fill=None):
            n = int(np.prod(shape))
            if parent is not None and getattr(parent, name, None) is not None:
                t = getattr(parent, name).reshape(-1)[:n].view(shape)
            else:
                fresh.add(name)
                if fill is None:
                    t = torch.empty(shape, dtype=dtype, device=dev)
                else:
                    t = torch.full(shape, fill, dtype=dtype, device=dev)
            setattr(self, name, t)
            return t

        fresh = set()   # buffers this workspace owns (not views of the parent's)

        self.plans = {}
        alloc('q', (N,), torch.int32)
        # the clean codes of a call whose network input differs from its
        # targets (loss / score with input_codes): ws.q is what the network
        # reads, q_tgt what the cross-entropy and scoring launches label with
        alloc('q_tgt', (N,), torch.int32)
        self.gc_ids = alloc('gc_ids', (B,), torch.int32) \
            if net.card is not None else None
        self.audio = alloc('audio', (N,)) if net.scalar_input else None
        alloc('X', (LP, N, CH))
        alloc('Z', (LP, N, CH))
        alloc('h1', (N, S))
        alloc('h2', (N, S))
        alloc('logits', (N, Q))
        alloc('bias_fg', (L, B, 2 * CHn))
        # persistent residual-stack kernels (wn_stack_fwd): one "rows are in
        # memory" flag per (layer, 32-row tile) and a 4-word control block
        # {group ticket, workgroups done, epoch, error}; epochs start at 1
        alloc('stack_flags', (lib.wn_stack_flag_count(B, T, L),), torch.int32,
              fill=0)
        alloc('wimg_f', (L, lib.wn_stack_wimg_floats()))
        alloc('stack_ctl', (4,), torch.int32, fill=0)
        if 'stack_ctl' in fresh:         # (a view shares the owner's epoch)
            self.stack_ctl[2] = 1
        alloc('bsum', (S,))
        self.total = alloc('total', (N, S)) if net.residual_postproc else None
        self.nparts = lib.wn_xent_partials(N)
        # (the first 2 words: the NaN "poison" of wn_stack_fwd / wn_stack_bwd,
        # summed into the loss with the partials that follow them: an expired
        # wait turns the loss NaN; in front so that a carved-out workspace
        # shares them)
        alloc('loss_parts', (2 + self.nparts,), fill=0.0)
        alloc('loss', (1,), fill=0.0)
        # masked loss (loss(lengths=...)): the clips' lengths and, in the last
        # word, the bits of float32 1 / denominator, staged per call; the
        # kernel reads them from here, so a replayed launch sees this call's
        alloc('xent_mask', (B + 1,), torch.int32, fill=0)
        # ... and the clips' history (loss(history=...)), staged the same way
        alloc('xent_hist', (B,), torch.int32, fill=0)
        alloc('proba', (Q,))
        lcond.alloc_workspace(net, self, alloc, None)
        if net.blocked:
            # partial pre-activations of a layer wider than one chunk of
            # channel blocks (wavenet/blocked.py), planes af | ag
            alloc('pre', (2 * CB, N, CH))
        if not training:
            return
        # the generic-tap / channel-block backward kernels also need the tanh
        # plane and two ping-pong pairs of pre-activation-gradient planes; the
        # default wn_stack_bwd / wn_layer_bwd2 do not
        self.legacy = net._layer_path() != 'layer'
        self.TH = alloc('TH', (LP, N, CH)) if self.legacy else None
        alloc('SG', (LP, N, CH))
        alloc('dZ', (LP, N, CH))
        alloc('dc1', (N, S))
        alloc('dtotal', (N, S))
        self.dh2 = alloc('dh2', (N, S)) if net.residual_postproc else None
        self.c1 = alloc('c1', (N, S)) if net.residual_postproc else None
        self.da = alloc('da', (2, 2 * CB, N, CH)) if self.legacy else None
        alloc('dx', (2, CB, N, CH))
        # persistent backward (wn_stack_bwd), "push" formulation: a tile's
        # own dx rows have no reader but the wave that wrote them, so ONE
        # plane is rewritten in place from layer to layer (it stays in the L2
        # / Infinity Cache; DX[0] ends up as dL/dx_0).  The per-layer checks of
        # tests/test_gpu_stack.py (`net.stack_bwd_keep_dx`) keep dL/dx_l of
        # EVERY layer.  Plus the q planes, flags and control block (allocated
        # whenever the option could apply)
        self.stack_bwd = bool(net.stack_bwd and net._stack_ok(N))
        if self.stack_bwd:
            self.keep_dx = bool(net.stack_bwd_keep_dx)
            if parent is not None and getattr(parent, 'DX', None) is not None:
                self.keep_dx = parent.keep_dx
            alloc('DX', (L if self.keep_dx else 1, N, CH))
            # q_l planes of the "push" formulation: what a tile's rows send to
            # the rows d earlier (csrc/wn_stack.hip)
            alloc('DQ', (L, N, CH))
            alloc('wimg_b', (L, lib.wn_stack_wimg_floats()))
            alloc('stack_flags_b', (lib.wn_stack_flag_count(B, T, L),),
                  torch.int32, fill=0)
            alloc('stack_ctl_b', (4,), torch.int32, fill=0)
            # a child whose parent was built without the backward stack
            # buffers owns fresh flags (all 0): its epoch must start at 1 too
            if 'stack_ctl_b' in fresh:
                self.stack_ctl_b[2] = 1
        if net.blocked:                  # channel-block path scratch
            alloc('dzb', (CB, N, CH))
            alloc('wdT', (CHn, CHn))
            alloc('blk_tmp', (max((2 * net.KW + 1) * 1024 + 96, Q * CH,
                                  net.initial_filter_width * CH),))
            alloc('cs_tmp', (B, 64))
        alloc('w2t', (Q, S))
        alloc('w1t', (S, S))
        alloc('wst', (S, L * CHn))
        # ---- slab regions, self.region[key], declared here and in
        # lcond.alloc_workspace
        shared = []

        def region(key, count, stride, n, own=None, side=False):
            """Declare SlabRegion `key` on a buffer of its own (`own`: its
            name) or on the shared scratch ws.slabs (side: and, as key +
            '_side', on ws.slabs_tn)."""
            if own:
                self.region[key] = SlabRegion(alloc(own, (count, stride)),
                                              count, stride, n)
            else:
                shared.append((key, count, stride, n, side))

        self.region = {}
        ntiles = B * ((T + 31) // 32)
        nslab = max(1, min(512, ntiles // 4))
        alloc('wimg', (L, lib.wn_layer_bwd2_wimg_floats()))
        if net.blocked:
            # channel-block path: one slab region per (input, output) block
            # pair of ONE layer (wavenet/blocked.py), summed by
            # wn_reduce_pair_slabs; the per-layer slabs of the 32-channel
            # kernels are not used.  The scratch grows with the SQUARE of the
            # block count (CB^2 x nslab x up to 17.5 K floats: 36 GB at 1024
            # channels and 8 taps with 512 slabs): fewer, longer row splits
            # beyond 8 GB instead of an opaque allocation failure
            pair = (2 * min(net.KW, 8) + 1) * 1024 + 96
            nslab = max(1, min(nslab, (8 << 30) // (CB * CB * pair * 4)))
            alloc('pslabs', (CB * CB, nslab, pair))
            self.region['pairs'] = SlabRegion(self.pslabs, nslab, pair, pair)
            alloc('lslabs', (1, 1, 4))
        else:
            # layer-block gradients [L][count][LAYER_BLOCK]: one buffer, as
            # many slabs per layer as the backward that runs writes (the
            # generic-tap kernels, wn_layer_bwd2, wn_stack_bwd)
            counts = dict(
                layers_k=nslab, layers_2=lib.wn_layer_bwd2_slabs(B, T),
                layers_stack=lib.wn_stack_bwd_slabs(B, T, self.stack_variant)
                if self.stack_bwd else 0)
            # (an owner also holds the slabs of its most demanding view, which
            # may take the backward stack when the owner itself does not)
            fit = _view_stack_slabs(lib, B, T, self.stack_variant) \
                if parent is None and net._stack_ok() else 0
            alloc('lslabs', (L, max(fit, *counts.values()), net.LAYER_BLOCK))
            for key, count in counts.items():
                self.region[key] = SlabRegion(
                    self.lslabs, count, net.LAYER_BLOCK,
                    net.LAYER_BLOCK if net.use_biases else net.LAYER_W)
        # the TN GEMMs' per-split slabs (matrix, then the column-sum tail
        # rows); `side`: a second region on ws.slabs_tn for the side stream
        for key, mw, nw in (('post2', S, Q), ('post1', S, S),
                            ('skip', L * CHn, S)):
            region(key, lib.wn_gemm_tn_splits(N, mw, nw, 0),
                   lib.wn_gemm_tn_slab_floats(mw, nw), mw * nw, side=True)
        # causal-layer wgrad: the one-hot TN GEMM of one tap, scalar input
        # ([splits][initial_filter_width][32], as many splits), or the
        # segmented sum over the codes ([slabs][2][Q][32])
        sp, K0 = lib.wn_gemm_tn_splits(N, Q, CH, 1), net.initial_filter_width
        region('causal_onehot', sp, lib.wn_gemm_tn_slab_floats(Q, CH), Q * CH)
        region('causal_scalar', sp, K0 * CH, K0 * CH)
        region('causal_segsum', lib.wn_causal_wgrad_slabs(N), 2 * Q * CH,
               2 * Q * CH)
        lcond.alloc_workspace(net, self, alloc, region)
        # ws.slabs is sized HERE and nowhere else: the largest region declared
        # on it.  Sharing is safe because every producer that writes a region
        # of ws.slabs runs on the MAIN stream, one after another, and the
        # region's wn_reduce_slabs is issued on that stream before the next
        # producer starts: at most one region is live at a time.  The side
        # stream (TN GEMMs beside the backward stack, StepPath.overlap_tn)
        # must not share it: its three regions live on ws.slabs_tn, under the
        # same rule on that stream.
        alloc('slabs', (max(c * s for _, c, s, _, _ in shared),))
        alloc('slabs_tn', (max(c * s for _, c, s, _, sd in shared if sd),))
        for key, count, stride, n, side in shared:
            self.region[key] = SlabRegion(self.slabs[:count * stride], count,
                                          stride, n)
            if side:
                self.region[key + '_side'] = SlabRegion(
                    self.slabs_tn[:count * stride], count, stride, n)
        self.ev_fork = torch.cuda.Event() if dev.type == 'cuda' else None
        self.ev_join = torch.cuda.Event() if dev.type == 'cuda' else None
        self.dsum = alloc('dsum', (L, B, 2 * CHn)) if net.G else None
        self.gc_part = alloc('gc_part', (L, B, net.G)) if net.G else None
        # per-tile column sums of da: [L][tiles][64] for 32-row tiles (the
        # per-layer kernels, wn_stack_bwd on big batches) or 16-row tiles
        # (wn_stack_bwd on small ones, wn_stack_tile_rows): two views of one buffer
        self.stack_rows = lib.wn_stack_tile_rows(B, T, self.stack_variant)
        nt16 = B * ((T + 15) // 16)
        if net.G:
            buf = alloc('tilesum_buf', (L * nt16 * 64,))
            self.tilesum = buf[:L * ntiles * 64].view(L, ntiles, 64)
            self.tilesum16 = buf.view(L, nt16, 64)
        else:
            self.tilesum = self.tilesum16 = None
        self.dsum_part = alloc(
            'dsum_part', (B * lib.wn_colsum_clip_chunks(T) * 64,)) \
            if net.G else None
        alloc('l2_parts', (lib.wn_l2_partials_count(),))
        alloc('l2', (1,), fill=0.0)


def _view_stack_slabs(lib, B, T, variant):
    """The most weight-gradient slabs per layer wn_stack_bwd writes at any
    (B, T') with T' <= T.  The count is not monotone in T': it drops where
    the launch goes from 16- to 32-row tiles and where a wave takes one more
    tile, so a view can need more slabs than its owner's own launch.  It
    depends on T' through ceil(T' / 16) and ceil(T' / 32) only: one question
    per 16 rows covers every shorter shape."""
    return max(lib.wn_stack_bwd_slabs(B, min(16 * k, T), variant)
               for k in range(1, (T + 15) // 16 + 1))


def get(net, B, T, training):
    """The model's workspace for (B, T), from its cache `net._ws`: the
    resident one, a view carved out of a larger one, or a new owner."""
    key = (B, T, bool(training))
    ws = net._ws.get(key)
    if ws is not None and training and net._layer_path() != 'layer' \
            and not ws.legacy:
        net._ws = {}          # switched to a legacy backward: re-allocate
        ws = None
    if ws is not None:
        return ws
    # carve out of a resident larger workspace of the same batch size
    for (b, t, tr), cand in list(net._ws.items()):
        if cand.capacity == cand.N and b == B and B * T <= cand.capacity \
                and (tr or not training):
            ws = _Workspace(net, B, T, training, parent=cand)
            break
    if ws is None:
        # grow geometrically (the naive generation path asks for T, T+1,
        # ... up to its window) and keep ONE owner per kind resident: a
        # training step and forward-only calls of another length do not
        # evict each other's buffers and launch plans
        prev = [w for (b, t, tr), w in net._ws.items()
                if w.capacity == w.N and tr == bool(training) and b == B]
        t_alloc = T
        if prev and not training:
            t_alloc = max(T, min(2 * max(w.T for w in prev), 1 << 20))
        net._ws = {k: w for k, w in net._ws.items()
                    if w.training != bool(training)}
        owner = _Workspace(net, B, t_alloc, training)
        net._ws[(B, t_alloc, bool(training))] = owner
        ws = owner if t_alloc == T else \
            _Workspace(net, B, T, training, parent=owner)
    net._ws[key] = ws
    if len(net._ws) > 64:        # views are cheap but unbounded otherwise
        owners = {k: v for k, v in net._ws.items()
                  if v.capacity == v.N}
        net._ws = owners
        net._ws[key] = ws
    return ws
