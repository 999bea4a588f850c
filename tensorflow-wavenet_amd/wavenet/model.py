"""WaveNetModel on MI355X: host-side mirror of the reference's
wavenet/model.py::WaveNetModel (same constructor signature :46-60, same
`variables` nesting/names/shapes :118-225, same public methods `loss` :628,
`predict_proba` :564, `predict_proba_incremental` :592) driving hand-written
HIP kernels through the C ABI of include/wavenet_hip.h.

MI355X-first design:
  * all parameters live in ONE flat fp32 device buffer (`params`), all
    gradients in ONE flat bucket (`grads`) -> one RCCL all-reduce, one fused
    optimizer launch; `variables[...]` are reference-shaped views into it;
  * activations are [B*T][32] planes; each residual block is one fused MFMA
    kernel; the 50 skip 1x1 convs are a single [B*T, L*32] x [L*32, S] GEMM;
  * the one-hot input tensor is never materialised (causal layer = gather,
    its weight gradient = one-hot-on-the-fly MFMA contraction);
  * backward is hand-written (the reference relies on TF autodiff).
There is no CPU / PyTorch compute fallback: without the HIP library or a GPU
every entry point raises.
"""
import math

import numpy as np
import torch

from . import _lib
from . import fastgen
from . import features
from . import local_condition as lcond
from . import mol
from . import sampling
from . import train_pass
from . import workspace
from .ops import mu_law_encode, mu_law_decode, mu_law_tables
from .workspace import CH

# layer block (floats) for filter width K and C = 32 * blocks padded channels:
#   Wf[K][C][C] Wg[K][C][C] Wd[C][C] bf[C] bg[C] bd[C] (+ gc weights [G][C] x 2)


def layer_w(K, C=CH):
    return (2 * K + 1) * C * C


def _align(n, a=32):
    return (n + a - 1) // a * a


def _xavier_(t, gen):
    """tf.contrib.layers.xavier_initializer_conv2d (uniform), model.py:10:
    limit sqrt(6 / (fan_in + fan_out)) with the receptive field folded in."""
    shape = tuple(t.shape)
    rf = int(np.prod(shape[:-2])) if len(shape) > 2 else 1
    lim = math.sqrt(6.0 / (rf * shape[-2] + rf * shape[-1]))
    vals = (torch.rand(shape, generator=gen, dtype=torch.float32) * 2 - 1) * lim
    t.copy_(vals.to(t.device))


def check_lengths(lengths, loss_denominator, B, T, what):
    """The `lengths` / `loss_denominator` of a loss call, checked on the host:
    None without lengths, else (lengths as int32 numpy [B], the denominator
    as a float: sum(lengths) unless the caller gave one)."""
    if lengths is None:
        if loss_denominator is not None:
            raise ValueError('%s: loss_denominator needs lengths' % what)
        return None
    n = features.check_lengths(lengths, B, T, what)
    den = float(n.astype(np.int64).sum())
    if loss_denominator is not None:
        d = loss_denominator
        if isinstance(d, (bool, np.bool_)) or \
                not isinstance(d, (int, float, np.integer, np.floating)) or \
                not np.isfinite(d) or not d > 0:
            raise ValueError('%s: loss_denominator must be a positive finite '
                             'number, got %r' % (what, d))
        den = float(d)
    return n, den


def receptive_field(dilations, filter_width, scalar_input=False,
                    initial_filter_width=32):
    """R: logits row t depends on input samples t - R + 1 .. t and on no
    earlier one.  A filter of K taps at dilation d reaches back s(K) * d
    samples, s(K) = (K - 1) + (K - 1) // 2 (the tap rule of
    csrc/wn_layer.hip, tap_shift); the causal layer has initial_filter_width
    taps with scalar_input, else filter_width.  Host arithmetic only."""
    def reach(K):
        return (int(K) - 1) + (int(K) - 1) // 2
    Kc = initial_filter_width if scalar_input else filter_width
    return 1 + reach(Kc) + reach(filter_width) * int(sum(dilations))


def check_history(history, mask, loss_denominator, B, T, what):
    """The `history` of a loss / score call, checked on the host: B ints (or
    one for all clips) with 0 <= history[b] <= n[b], n[b] = lengths[b] or T.
    Returns (mask, history as int32 numpy [B]); (mask, None) without history.
    The mask always carries lengths then (T for every clip without them), and
    its denominator is sum(n - history) unless the caller gave one."""
    if history is None:
        return mask, None
    h = history
    if hasattr(h, 'detach'):
        h = h.detach().cpu().numpy()
    h = np.asarray(h)
    if h.dtype == object or h.dtype == np.bool_ or \
            not np.issubdtype(h.dtype, np.integer):
        raise ValueError('%s: history must be an integer or %d integers '
                         '(dtype %s)' % (what, B, h.dtype))
    if h.shape not in ((), (B,)):
        raise ValueError('%s: history must be one int or have shape [%d], '
                         'got %s' % (what, B, list(h.shape)))
    h = np.broadcast_to(h.astype(np.int64), (B,))
    n = np.full(B, T, np.int64) if mask is None else mask[0].astype(np.int64)
    if (h < 0).any() or (h > n).any():
        raise ValueError('%s: history must lie in [0, n[b]], n = %s, got %s'
                         % (what, n.tolist(), h.tolist()))
    total = int((n - h).sum())
    # (a caller that gives the denominator -- a data-parallel rank -- may
    # hold clips without a target while another rank holds some)
    if total == 0 and (mask is None or loss_denominator is None):
        raise ValueError('%s: history leaves no sample to predict: '
                         'sum(n - history) is 0' % what)
    den = float(total) if mask is None or loss_denominator is None \
        else mask[1]
    return (n.astype(np.int32), den), h.astype(np.int32)


def _n_codes(codes):
    """Number of codes of a seed (None: the one default code)."""
    if codes is None:
        return 1
    if isinstance(codes, torch.Tensor):
        return int(codes.numel())
    return int(np.asarray(codes).size)


class WaveNetModel(object):
    '''Implements the WaveNet network for generative audio (MI355X / HIP).

    Usage mirrors the reference (model.py:31-44):
        net = WaveNetModel(batch_size, dilations, filter_width,
                           residual_channels, dilation_channels, skip_channels)
        loss = net.loss(input_batch)          # forward + backward on the GPU
        optimizer.minimize(loss)              # fused TF-rule update
    '''

    # variant word of the stack launches a new model starts with (0 = the
    # library's choice per shape; tests / tools set it, see `stack_variant`)
    DEFAULT_STACK_VARIANT = 0

    def __init__(self,
                 batch_size,
                 dilations,
                 filter_width,
                 residual_channels,
                 dilation_channels,
                 skip_channels,
                 quantization_channels=2**8,
                 use_biases=False,
                 scalar_input=False,
                 initial_filter_width=32,
                 histograms=False,
                 global_condition_channels=None,
                 global_condition_cardinality=None,
                 residual_postproc=False,
                 device=None,
                 seed=0,
                 *,
                 local_condition_channels=None,
                 local_condition_upsample_scales=None,
                 local_condition_context=None,
                 output_mixture=None,
                 mixture_log_scale_min=-14.0):
        # mixture-of-logistics head over 65536 levels (wavenet/mol.py):
        # output_mixture=K components, 3 Kp output columns [pi | mu | beta_raw]
        # in the place of the softmax's quantization_channels, which the
        # network then does not read
        self.output_mixture = output_mixture
        self.mixture_log_scale_min = mixture_log_scale_min
        self.mol_K = self.mol_Kp = 0
        if output_mixture is not None:
            self.mol_K, self.mol_log_scale_min = mol.check_config(
                output_mixture, mixture_log_scale_min, scalar_input)
            self.mol_Kp = mol.padded(self.mol_K)
        self.batch_size = batch_size
        self.dilations = list(dilations)
        self.filter_width = filter_width
        self.residual_channels = residual_channels
        self.dilation_channels = dilation_channels
        self.quantization_channels = quantization_channels
        self.use_biases = use_biases
        self.skip_channels = skip_channels
        self.scalar_input = scalar_input
        self.initial_filter_width = initial_filter_width
        self.histograms = histograms
        self.global_condition_channels = global_condition_channels
        self.global_condition_cardinality = global_condition_cardinality
        self.residual_postproc = residual_postproc
        # local conditioning (WaveNet paper 2.5): per-sample features lc[b, t]
        # of this many channels, see `loss` / `predict_proba`
        lcond.configure(self, local_condition_channels,
                        local_condition_upsample_scales,
                        local_condition_context)
        # TF's fused softmax-xent back-propagates softmax/(B*T) through the
        # all-zero-label last row of every clip [inferred].
        self.tf_xent_zero_label_quirk = True
        # model.py:28 passes the bias *name* as `trainable`, so the reference's
        # L2 filter "'bias' in v.name" (model.py:676) does not exclude biases.
        self.tf_bias_name_quirk = True
        # Run the three weight-gradient (TN) GEMMs of the skip / post-processing
        # convs on a second, lower-priority HIP stream next to the dZ GEMM and
        # the residual-stack backward (one fork after the dtotal GEMM, one join
        # before the slab reductions): the layer kernels keep the matrix pipes
        # about a third busy, the TN GEMMs are MFMA-bound.  None (default):
        # on for small batches only -- at most four 32-row tiles per CU, where
        # the backward stack is one dependent chain per tile that leaves most
        # of the chip idle (B = 1, T = 16000: 2.03 -> 1.88 ms per step; B = 2:
        # 2.94 -> 2.89; neutral at B = 4, 1 % SLOWER at B = 8).  True / False
        # force it.
        self.overlap_tn = None
        # channel-block models (33 - 128 channels): dz and the gate gradients
        # in one launch (False: two launches, A/B and tests; bitwise equal)
        self.wide_fuse_gate = True
        # forward of the residual stack as ONE persistent launch
        # (wn_stack_fwd: tiles stay in registers from layer to layer, the
        # dilated taps are handed over through per-tile flags) instead of one
        # wn_layer_fwd launch per layer.  False selects the latter.
        self.stack_fwd = True
        # ... with the skip sum inside that launch where the library has it
        # (wn_stack_fwd_skip: small batches, 512 skip channels)
        self.stack_fwd_skip = True
        # the same for the backward of the stack (wn_stack_bwd instead of one
        # wn_layer_bwd2 per layer); read when a workspace is created
        self.stack_bwd = True
        # diagnostic: keep dL/dx_l of every layer instead of one plane
        # rewritten in place (read when a workspace is created)
        self.stack_bwd_keep_dx = False
        # explicit variant word of the stack launches (_lib.stack_variant:
        # tile rows, waves per workgroup, split backward), 0 = the library's
        # choice for the shape; for A/B runs and tests, read when a workspace
        # is created (setting it drops the resident workspaces).  (The library
        # reads no process environment.)
        self._stack_variant = int(self.DEFAULT_STACK_VARIANT)
        # data-parallel runs (wavenet/parallel.py): start the all-reduce of the
        # skip / post-processing gradients -- 82 % of the bucket, complete
        # before the backward stack launch -- from inside the backward pass,
        # on a communication stream beside that launch.  Opt-in (train.py
        # --dp_overlap_allreduce; bench.py times it as a trial): whoever
        # switches it on promises that optimizer.minimize (which joins)
        # follows every loss().  Ignored outside torch.distributed and when L2
        # regularisation is on.
        self.dp_overlap_allreduce = False
        self._tail_work = None
        # generate(): four kernels per sample over many CUs, replayed from a
        # hipGraph, instead of the single-workgroup persistent kernel
        self.fastgen_multi_cu = True
        self.fastgen_graph_steps = 200
        # the multi-CU path as ONE persistent launch per generate() call
        # (wn_fastgen_persist: chain segments / skip / post-processing / draw
        # workgroups resident for the whole run, weights resident in LDS,
        # in-launch hand-overs instead of four kernel boundaries per sample);
        # False: the step kernels replayed from a hipGraph
        self.fastgen_persistent = True
        # persistent / cooperative generation launches that expired once on this
        # device (CUs held elsewhere): not tried again by any generator of this
        # model; `reset_generator_launch_failures()` clears it
        self._gen_launch_failed = {}
        # 64-channel models: wn_fastgen_run_wide's cooperative launch
        self.fastgen_wide_coop = True
        # 'fp32' (default): fp32 MFMA GEMMs.  'bf16x6' / 'bf16x9' / 'bf16x3':
        # opt-in split-bf16 products for the six NN GEMMs (wn_gemm_nn_split;
        # x6 measures the same error vs float64 as the fp32 MFMA path)
        self.gemm_mode = 'fp32'
        self._wsplit = {}
        # replay recorded (function, args) launch sequences instead of
        # re-deriving ~235 argument lists per step in Python
        self.use_launch_plans = True
        # bench.py's live roofline: a list collects (start, end, flops, name)
        # HIP events of the timed launches (_lib.call_timed); None: untimed
        self._gemm_events = None
        # seeds longer than this are primed from ONE batch forward pass
        # instead of one incremental step per seed sample
        self.fastgen_prime_forward_min = 64
        # LC models: steps per chunk of a fast-generation call (the
        # conditioned-bias ring holds chunk + 1 rows); None: as many as
        # fastgen.LC_RING_BYTES holds, a multiple of fastgen_graph_steps
        self.fastgen_lc_chunk = None

        _lib.load()
        if device is None:
            _lib.require_gpu()
            self.device = torch.device('cuda', torch.cuda.current_device())
        else:
            # device='cpu' is allowed for parameter bookkeeping only (variable
            # names / shapes / checkpoints); every compute entry point raises.
            self.device = torch.device(device)
        self.L, self.S, self.Q = len(self.dilations), skip_channels, \
            3 * self.mol_Kp if self.mol_K else quantization_channels
        self.R, self.D = residual_channels, dilation_channels
        self.G = global_condition_channels
        self.card = global_condition_cardinality
        self._unsupported = None
        if filter_width < 2 or filter_width > 64:
            # (above 8 the layers run in groups of 8 taps, wavenet/blocked.py;
            # tested at 11 and 19)
            self._unsupported = 'filter_width must be in [2, 64] on the HIP path'
        elif max(self.R, self.D) > 1024:
            # channel-block kernels (wavenet/blocked.py): 32-wide blocks, in
            # chunks of 8 // filter_width blocks per kernel call; tested up to
            # 320 channels, capped at 32 blocks
            self._unsupported = ('at most 1024 residual / dilation channels on '
                                 'the HIP path')
        elif self.S % 4 or self.Q % 4:
            self._unsupported = 'skip/quantization channels must be multiples of 4'
        elif self.G is not None and self.card is None:
            self._unsupported = ('dense-vector global conditioning cannot run in '
                                 'the reference either (model.py:547,553)')
        self.KW = K = int(filter_width)
        # more than 32 residual / dilation channels: 32-wide channel blocks,
        # one activation plane per block (wavenet/blocked.py)
        self.CB = max(1, (max(self.R, self.D) + CH - 1) // CH)
        self.CHn = C = CH * self.CB
        # K = 2 runs the tuned kernels; other widths (or forcing it, for
        # tests) the generic-tap kernels
        self.generic_layers = K != 2
        # channel-block kernels (wavenet/blocked.py): more than 32 channels, or
        # a filter wider than the generic-tap kernels' 8 taps
        self.blocked = self.CB > 1 or K > 8
        self.LAYER_W = layer_w(K, C)
        self.OFF_BF = self.LAYER_W
        self.OFF_BG = self.LAYER_W + C
        self.OFF_BD = self.LAYER_W + 2 * C
        self.LAYER_BLOCK = self.LAYER_W + 3 * C
        self.OFF_GC = self.LAYER_BLOCK
        self._ws = {}
        self._dil_dev = torch.tensor(self.dilations, dtype=torch.int32,
                                     device=self.device)
        self._gen = None
        self._bgen = None
        self.init_ops = []
        self.push_ops = []
        self.variables = self._create_variables(seed)

    # local conditioning's limits (checked in wavenet/local_condition.py)
    LC_SUPPORTED = ('local conditioning is supported for residual / dilation '
                    'channels <= 32, filter_width 2 and one-hot input, or '
                    'scalar_input with a mixture-of-logistics head '
                    '(output_mixture: training, scoring, predict_mixture and '
                    'generate_mixture_batch), on the persistent stack '
                    'launches (stack_fwd / stack_bwd = True)')
    LC_UPSAMPLE_MAX_LAYERS = 8
    LC_UPSAMPLE_MAX_HOP = 4096
    LC_UPSAMPLE_MAX_CHANNELS = 512     # wn_lc_upsample_* (LCUP_MAX_LC)
    LC_CONTEXT_MAX = 8                 # wn_lc_context_* (LCCTX_MAX_P)
    # (LC checks under the names the host tests call them by)
    _lc_rows = lcond.rows
    _lc_input = lcond.check
    _lc_frames = lcond.frames
    _lc_forward_ok = lcond.forward_ok

    @property
    def receptive_field(self):
        """The model's receptive field in samples (receptive_field above):
        5117 for the default stack.  Needs no library and no device."""
        return receptive_field(self.dilations, self.filter_width,
                               self.scalar_input, self.initial_filter_width)

    @property
    def stack_variant(self):
        return self._stack_variant

    def _stack_variant_for_launch(self):
        """The variant word the stack launches of a new workspace get: an LC
        model always runs the 32-row launches (wn_stack_fwd_lc / _bwd_lc)."""
        v = int(self._stack_variant)
        return (v & ~0x3f) | 32 if self.Lc else v

    @stack_variant.setter
    def stack_variant(self, v):
        if int(v) != self._stack_variant:
            self._stack_variant = int(v)
            self._ws = {}          # slab counts / tile sums depend on it

    # ------------------------------------------------------------------ params
    def _create_variables(self, seed):
        '''Creates all variables (model.py:118-225) as views into one flat
        buffer; same nesting, keys and [K, Cin, Cout] shapes as the reference.'''
        L, S, Q, R, D, G, card = (self.L, self.S, self.Q, self.R, self.D,
                                  self.G, self.card)
        if self._unsupported:
            self.params = torch.zeros(4, device=self.device)
            self.grads = torch.zeros(4, device=self.device)
            return {}
        C = self.CHn
        self.layer_stride = self.LAYER_BLOCK + (2 * G * C if G else 0)
        seg, off = {}, 0
        def add(name, n):
            nonlocal off
            seg[name] = (off, n)
            off = _align(off + n)
        if card is not None:
            add('emb', card * G)
        add('causal', (self.initial_filter_width if self.scalar_input
                       else self.KW * Q) * C)
        add('layers', L * self.layer_stride)
        if self.Lc:
            # local conditioning: [Lcp][L][64] (filter | gate columns of every
            # layer next to each other, the addend GEMM's weight as it is).  In
            # front of skip_w: the data-parallel tail all-reduce starts there
            # (parallel.tail_start) before this gradient exists
            add('lc_w', self.Lcp * L * 64)
        if self.lc_up:
            # the upsampler: filters [s_i][3] of every layer, then (biases)
            # one scalar per layer.  Also in front of skip_w
            add('lc_up', lcond.up_floats(self))
        if self.lc_ctx is not None:
            # the frame-context filter [2p + 1][Lc][Lc].  Also in front of
            # skip_w
            add('lc_ctx', (2 * self.lc_ctx + 1) * self.Lc * self.Lc)
        add('skip_w', L * C * S)
        add('skip_b', L * S)
        add('post1_w', S * S)
        add('post2_w', S * Q)
        add('post1_b', S)
        add('post2_b', Q)
        self.segments = seg
        self.params = torch.zeros(off, dtype=torch.float32, device=self.device)
        self.grads = torch.zeros_like(self.params)
        self.variables = self._views(self.params)
        self.gradients = self._views(self.grads)
        self._init_variables(seed)
        return self.variables

    def _seg(self, flat, name):
        o, n = self.segments[name]
        return flat[o:o + n]

    def _views(self, flat):
        L, S, Q, R, D, G, card = (self.L, self.S, self.Q, self.R, self.D,
                                  self.G, self.card)
        var = dict()
        CH = self.CHn              # padded channel count of every weight
        if card is not None:
            var['embeddings'] = {
                'gc_embedding': self._seg(flat, 'emb').view(card, G)}
        if self.scalar_input:                               # model.py:143-153
            var['causal_layer'] = {'filter': self._seg(flat, 'causal').view(
                self.initial_filter_width, 1, CH)[:, :, :R]}
        else:
            var['causal_layer'] = {
                'filter': self._seg(flat, 'causal').view(self.KW, Q, CH)[
                    :, :, :R]}
        layers = self._seg(flat, 'layers').view(L, self.layer_stride)
        skw = self._seg(flat, 'skip_w').view(L, 1, CH, S)
        skb = self._seg(flat, 'skip_b').view(L, S)
        lcw = self._seg(flat, 'lc_w').view(self.Lcp, L, 64) if self.Lc else None
        var['dilated_stack'] = []
        for i in range(L):
            blk = layers[i]
            cur = dict()
            K = self.KW
            OFF_GC, OFF_BF, OFF_BG, OFF_BD = (self.OFF_GC, self.OFF_BF,
                                              self.OFF_BG, self.OFF_BD)
            M = CH * CH
            cur['filter'] = blk[0:K * M].view(K, CH, CH)[:, :R, :D]
            cur['gate'] = blk[K * M:2 * K * M].view(K, CH, CH)[:, :R, :D]
            cur['dense'] = blk[2 * K * M:(2 * K + 1) * M].view(
                1, CH, CH)[:, :D, :R]
            cur['skip'] = skw[i][:, :D, :]
            if G is not None:
                gcf = blk[OFF_GC:OFF_GC + G * CH].view(1, G, CH)
                gcg = blk[OFF_GC + G * CH:OFF_GC + 2 * G * CH].view(1, G, CH)
                cur['gc_gateweights'] = gcg[:, :, :D]
                cur['gc_filtweights'] = gcf[:, :, :D]
            if lcw is not None:                 # [Lc, dilation_channels]
                cur['lc_filtweights'] = lcw[:self.Lc, i, :D]
                cur['lc_gateweights'] = lcw[:self.Lc, i, 32:32 + D]
            if self.use_biases:
                cur['filter_bias'] = blk[OFF_BF:OFF_BF + D]
                cur['gate_bias'] = blk[OFF_BG:OFF_BG + D]
                cur['dense_bias'] = blk[OFF_BD:OFF_BD + R]
                cur['skip_bias'] = skb[i]
            var['dilated_stack'].append(cur)
        if self.lc_up:
            # the upsampler, layer i: filter [s_i][3] (slot, tap), bias [1]
            up, fo, nf = self._seg(flat, 'lc_up'), 0, 3 * sum(self.lc_up)
            var['lc_upsample'] = []
            for i, s in enumerate(self.lc_up):
                cur = {'filter': up[fo:fo + 3 * s].view(s, 3)}
                if self.use_biases:
                    cur['bias'] = up[nf + i:nf + i + 1]
                var['lc_upsample'].append(cur)
                fo += 3 * s
        if self.lc_ctx is not None:
            var['lc_context'] = {'filter': self._seg(flat, 'lc_ctx').view(
                2 * self.lc_ctx + 1, self.Lc, self.Lc)}
        post = dict()
        post['postprocess1'] = self._seg(flat, 'post1_w').view(1, S, S)
        post['postprocess2'] = self._seg(flat, 'post2_w').view(1, S, Q)
        if self.use_biases:
            post['postprocess1_bias'] = self._seg(flat, 'post1_b')
            post['postprocess2_bias'] = self._seg(flat, 'post2_b')
        var['postprocessing'] = post
        return var

    def _init_variables(self, seed):
        """Xavier / identity / zero initialisation (model.py:7-28) drawn on the
        host into a flat staging buffer of the same layout and uploaded ONCE
        (not one small copy per variable)."""
        gen = torch.Generator().manual_seed(int(seed))
        host = torch.zeros(self.params.numel(), dtype=torch.float32)
        v = self._views(host)
        with torch.no_grad():
            if self.card is not None:
                e = v['embeddings']['gc_embedding']
                if self.card == self.G:                      # model.py:16-19
                    e.copy_(torch.eye(self.card))
                else:
                    _xavier_(e, gen)
            _xavier_(v['causal_layer']['filter'], gen)
            for cur in v['dilated_stack']:
                for k in ['filter', 'gate', 'dense', 'skip', 'gc_gateweights',
                          'gc_filtweights']:
                    if k in cur:
                        _xavier_(cur[k], gen)
            _xavier_(v['postprocessing']['postprocess1'], gen)
            _xavier_(v['postprocessing']['postprocess2'], gen)
            # (drawn last: every other variable gets the values it has in the
            # same model without LC)
            for cur in v['dilated_stack']:
                for k in ['lc_filtweights', 'lc_gateweights']:
                    if k in cur:
                        _xavier_(cur[k], gen)
            # the upsampler starts as repetition: W_i[j] = (0, 1, 0), b_i = 0
            # (no draws: every other variable keeps its values)
            for cur in v.get('lc_upsample', []):
                cur['filter'][:, 1] = 1.0
            # the context filter starts as the identity: centre tap I, the
            # others zero (no draws either)
            if 'lc_context' in v:
                v['lc_context']['filter'][self.lc_ctx] = torch.eye(self.Lc)
            # biases: zeros (model.py:27)
            self.params.copy_(host)

    def histogram_summaries(self, bins=30):
        """Counterpart of the `histograms=True` summaries of
        _create_dilation_layer (model.py:314-325): per layer, histograms of the
        filter / gate / dense (not for the last layer) / skip weights and,
        with biases, of the four bias vectors, under the reference's tags
        (`layer3_filter`, `layer3_biases_gate`, ...).  Returns
        {tag: (counts int64[bins], lo, hi)}; empty unless the model was built
        with histograms=True."""
        out = {}
        if not self.histograms:
            return out
        L = self.L
        tags = [('filter', '_filter'), ('gate', '_gate'), ('dense', '_dense'),
                ('skip', '_skip'), ('filter_bias', '_biases_filter'),
                ('gate_bias', '_biases_gate'), ('dense_bias', '_biases_dense'),
                ('skip_bias', '_biases_skip')]
        for i, cur in enumerate(self.variables['dilated_stack']):
            for k, suffix in tags:
                if k not in cur or (k == 'dense' and i == L - 1):
                    continue
                v = cur[k].detach().float().reshape(-1)
                lo, hi = float(v.min()), float(v.max())
                if hi <= lo:
                    hi = lo + 1e-12
                counts = torch.histc(v, bins=bins, min=lo, max=hi)
                out['layer%d%s' % (i, suffix)] = (
                    counts.to(torch.int64).cpu().numpy(), lo, hi)
        return out

    def named_variables(self, tree=None, prefix='wavenet'):
        """(reference variable name, view) pairs, creation order."""
        tree = self.variables if tree is None else tree
        out = []
        if 'embeddings' in tree:
            out.append((prefix + '/embeddings/gc_embedding',
                        tree['embeddings']['gc_embedding']))
        out.append((prefix + '/causal_layer/filter',
                    tree['causal_layer']['filter']))
        order = ['filter', 'gate', 'dense', 'skip', 'gc_gateweights',
                 'gc_filtweights', 'lc_gateweights', 'lc_filtweights',
                 'filter_bias', 'gate_bias', 'dense_bias', 'skip_bias']
        tfname = {'gc_gateweights': 'gc_gate', 'gc_filtweights': 'gc_filter',
                  'lc_gateweights': 'lc_gate', 'lc_filtweights': 'lc_filter',
                  'skip_bias': 'slip_bias'}       # sic, model.py:183-204
        for i, cur in enumerate(tree['dilated_stack']):
            for k in order:
                if k in cur:
                    out.append(('%s/dilated_stack/layer%d/%s'
                                % (prefix, i, tfname.get(k, k)), cur[k]))
        for i, cur in enumerate(tree.get('lc_upsample', [])):
            for k in ['filter', 'bias']:
                if k in cur:
                    out.append(('%s/lc_upsample/layer%d/%s' % (prefix, i, k),
                                cur[k]))
        if 'lc_context' in tree:
            out.append((prefix + '/lc_context/filter',
                        tree['lc_context']['filter']))
        for k in ['postprocess1', 'postprocess2', 'postprocess1_bias',
                  'postprocess2_bias']:
            if k in tree['postprocessing']:
                out.append((prefix + '/postprocessing/' + k,
                            tree['postprocessing'][k]))
        return out

    def state_dict(self):
        return {n: v.detach().cpu().clone() for n, v in self.named_variables()}

    def load_state_dict(self, sd):
        with torch.no_grad():
            for n, v in self.named_variables():
                v.copy_(torch.as_tensor(sd[n]).to(self.device))
        self._gen = None
        self._bgen = None

    def load_nested(self, tree):
        """Load a nested dict shaped like `variables` (numpy / tensors)."""
        def rec(dst, src):
            if isinstance(dst, dict):
                for k in dst:
                    rec(dst[k], src[k])
            elif isinstance(dst, list):
                for a, b in zip(dst, src):
                    rec(a, b)
            else:
                dst.copy_(torch.as_tensor(np.asarray(src),
                                          dtype=torch.float32).to(self.device))
        with torch.no_grad():
            rec(self.variables, tree)
        self._gen = None
        self._bgen = None

    # ------------------------------------------------------------------ helpers
    def _overlap_tn_on(self, ws):
        if self.overlap_tn is not None:
            return bool(self.overlap_tn)
        return ws.B * ((ws.T + 31) // 32) <= 1024 and not self.blocked

    def _layer_path(self):
        """The per-layer kernels: 'blocked' (channel blocks), 'layer_k'
        (generic taps, or `generic_layers` forced) or 'layer' (two taps, which
        alone can run the persistent stack launches instead)."""
        return 'blocked' if self.blocked else \
            'layer_k' if self.generic_layers else 'layer'

    def _stack_ok(self, N=None):
        """The persistent stack launches cover the model's layers and, given
        N = B * T, its rows (the backward's 32-bit plane offsets)."""
        return (self._layer_path() == 'layer' and self.L <= 256 and
                (N is None or N * CH * 4 < 2 ** 31))

    def _stack_bwd_ok(self):
        """wn_stack_bwd covers what wn_layer_bwd2 covers."""
        return bool(self.stack_bwd and self._stack_ok())

    def check_device_errors(self):
        """Raise if a persistent stack launch recorded an expired dependency
        wait (its control word 3; the loss of that step is NaN by
        construction, see workspace.py, loss_parts).  Synchronises the device:
        meant for the moment a caller sees a non-finite loss."""
        for ws in self._ws.values():
            for name in ('stack_ctl', 'stack_ctl_b'):
                ctl = getattr(ws, name, None)
                if ctl is not None and int(ctl[3]) != 0:
                    raise _lib.WaveNetHipError(
                        '%s: a dependency wait inside the persistent residual-'
                        'stack launch expired (2 s); the results of that step '
                        'are invalid.  net.stack_fwd / net.stack_bwd = False '
                        'select the one-launch-per-layer kernels.' % name)

    def reset_generator_launch_failures(self):
        """Try the persistent / cooperative generation launches again."""
        self._gen_launch_failed = {}

    def reset_device_errors(self):
        """Clear the expired-wait record (control word 3 and the NaN poison
        words) of every workspace, e.g. after a caller has handled the error
        `check_device_errors` raised."""
        for ws in self._ws.values():
            for name in ('stack_ctl', 'stack_ctl_b'):
                ctl = getattr(ws, name, None)
                if ctl is not None:
                    ctl[3] = 0
            ws.loss_parts[:2] = 0.0

    def _check_supported(self):
        if self._unsupported:
            raise NotImplementedError(self._unsupported)
        if self.device.type != 'cuda':
            raise _lib.WaveNetHipError(
                'WaveNetModel compute needs an MI355X (device=%s); there is '
                'no CPU fallback' % self.device)

    def _workspace(self, B, T, training):
        return workspace.get(self, B, T, training)

    def _step_path(self, ws, backward, l2=False):
        return train_pass.step_path(self, ws, backward, l2)

    def reserve(self, batch_size, max_samples, training=False):
        """Allocate the workspace for up to `max_samples` samples per clip now
        (generate.py's window, train.py's sample_size), so that later calls
        with shorter inputs carve views out of it instead of allocating."""
        self._check_supported()
        return self._workspace(int(batch_size), int(max_samples), training)

    def _gc_ids(self, global_condition, B):
        if self.card is None or global_condition is None:
            if self.G is not None and self.card is not None:
                raise ValueError('model was built with global conditioning; '
                                 'a global_condition id batch is required')
            return None
        ids = global_condition
        if not isinstance(ids, torch.Tensor):
            ids = torch.as_tensor(np.asarray(ids))
        ids = ids.reshape(-1).to(device=self.device, dtype=torch.int32)
        if ids.numel() != B:
            raise ValueError('global_condition has %d ids, batch_size is %d'
                             % (ids.numel(), B))
        return ids.contiguous()

    def upsample_local_condition(self, frames, num_samples, offset=0):
        """The learned upsampler on frame-rate features: frames float
        [B, F, Lc] (or [F, Lc]) -> device float32 rows [B, num_samples, Lc]
        (or [num_samples, Lc]); row t is timeline position offset[b] + t
        (offset: an int or B non-negative ints).  The same kernel as the
        training forward: a row's bits depend on its frame, its slot and the
        weights only.  The rows feed predict_proba and fast generation."""
        return lcond.upsample(self, frames, num_samples, offset)

    def local_condition_from_audio(self, spec, audio, lengths=None):
        """What this model's LC inputs take, computed from the audio by the
        log-mel front end `spec` (a features.MelSpec with n_mels = the
        model's LC channels): audio [B, T] or [T], lengths as for `loss`.
        A model built with local_condition_upsample_scales gets the frames
        [B, F, Lc], F = ceil(T / hop) (spec.hop must be the model's hop):
        pass them as local_condition_batch with local_condition_offset=0.
        A repetition-row model gets rows [B, T, Lc]: frame t // spec.hop
        beside sample t.  A device tensor, no host synchronisation."""
        return features.local_condition_from_audio(self, spec, audio, lengths)

    def _layer_block(self, flat, l):
        o, _ = self.segments['layers']
        return flat[o + l * self.layer_stride: o + (l + 1) * self.layer_stride]

    # ------------------------------------------------------------------ API
    def encode(self, input_batch, B=None):
        """mu-law codes [B, T] of float audio (model.py:639-640)."""
        B = self.batch_size if B is None else B
        a = input_batch
        if not isinstance(a, torch.Tensor):
            a = torch.as_tensor(np.asarray(a), dtype=torch.float32)
        a = a.to(device=self.device, dtype=torch.float32).reshape(B, -1)
        return mu_law_encode(a, self.Q)

    def loss(self,
             input_batch,
             global_condition_batch=None,
             l2_regularization_strength=None,
             name='wavenet',
             backward=True,
             *,
             local_condition_batch=None,
             local_condition_offset=0,
             lengths=None,
             loss_denominator=None,
             history=None,
             input_noise=None,
             noise_keys=None):
        '''Creates a WaveNet network and returns the autoencoding loss
        (model.py:628-685).  input_batch: float audio in [-1, 1], anything
        reshapeable to [batch_size, -1].  With backward=True (default) the
        gradient of the returned loss w.r.t. every variable is left in
        `self.grads` (the flat bucket `optimizer.minimize` consumes).

        local_condition_batch (models built with local_condition_channels=Lc,
        required there and refused elsewhere): float [batch_size, T, Lc] at
        audio rate.  Row t sits beside input sample t; the output at t is the
        distribution of sample t + 1, so row t conditions the prediction of
        sample t + 1.  Frame-rate features are upsampled by repetition first.

        Models built with local_condition_upsample_scales take FRAMES
        instead: float [batch_size, F, Lc], upsampled on the device by the
        learned network (gradients flow into it).  local_condition_offset
        (an int or batch_size non-negative ints, default 0): input sample t
        of clip b sits at timeline position offset[b] + t, which takes frame
        (offset[b] + t) // hop; F must cover offset[b] + T - 1.

        lengths (batch_size ints, 1 <= lengths[b] <= T): the batch is right
        padded and clip b has lengths[b] real samples.  Clip b is treated as
        a clip of T = lengths[b] fed alone: rows t + 1 < lengths[b] have the
        target q[b][t + 1], row lengths[b] - 1 is the label-less last row,
        rows t >= lengths[b] add nothing to the loss or to any gradient, and
        the mean is taken over sum(lengths) rows instead of batch_size * T.
        What the padding holds (audio, conditioning rows or frames) does not
        matter.  loss_denominator (a positive number, only with lengths)
        replaces sum(lengths): data-parallel ranks pass
        parallel.masked_denominator, so that their averaged gradient is the
        masked mean over the global batch.

        history (batch_size ints or one int, 0 <= history[b] <= n[b] with
        n[b] = lengths[b], or T without lengths): the first history[b]
        samples of clip b are fed to the network but predicted by nobody.
        Clip b is the clip of n[b] samples fed alone, as above; row t has a
        target iff history[b] <= t + 1 < n[b]; rows with t + 1 < history[b]
        add nothing to the loss or to any gradient; row n[b] - 1 stays the
        label-less last row; the mean is taken over sum(n - history) rows
        (loss_denominator still replaces it).  history = 0 is the call
        without history, bit for bit.

        input_noise (an input_noise.InputNoise) with noise_keys (batch_size
        ints in [0, 2**40) or a device int64 tensor; both or neither): the
        network reads perturbed codes -- each of clip b's n[b] input codes,
        history included, moved as InputNoise states with the key
        noise_keys[b] -- while every target stays the clean code.  One fused
        launch encodes the audio and perturbs it.  Not for scalar_input
        models, whose network input is the float audio.

        A model built with output_mixture=K (wavenet/mol.py) snaps the audio
        to 65536 levels on the device, reads their centres and is trained on
        the discretised mixture-of-logistics likelihood of level j[t + 1] in
        the place of the cross-entropy; everything above holds unchanged.'''
        self._check_noise(input_noise, noise_keys, 'loss')
        self._check_supported()
        B = self.batch_size
        a = input_batch
        if not isinstance(a, torch.Tensor):
            a = torch.as_tensor(np.asarray(a), dtype=torch.float32)
        a = a.to(device=self.device, dtype=torch.float32).reshape(B, -1)
        mask = check_lengths(lengths, loss_denominator, B, a.shape[1], 'loss')
        mask, hist = check_history(history, mask, loss_denominator, B,
                                   a.shape[1], 'loss')
        lc = lcond.check(self, local_condition_batch, local_condition_offset,
                         B, a.shape[1], 'loss')
        if self.mol_K:
            # centres into ws.audio, levels where the labels go
            ws = self._workspace(B, a.shape[1], backward)
            mol.stage(self, ws, a, mask)
            return self._loss(ws.q.view(B, -1), global_condition_batch,
                              l2_regularization_strength, backward, ws.audio,
                              lc, mask, hist)
        if input_noise is None:
            q, q_in = mu_law_encode(a, self.Q), None
        else:
            q, q_in = self._encode_noisy(a, input_noise, noise_keys, mask,
                                         backward)
        return self._loss(q, global_condition_batch,
                          l2_regularization_strength, backward, a, lc, mask,
                          hist, q_in)

    def loss_from_codes(self, q, global_condition_batch=None,
                        l2_regularization_strength=None, backward=True,
                        audio=None, *, local_condition_batch=None,
                        local_condition_offset=0, lengths=None,
                        loss_denominator=None, history=None,
                        input_codes=None):
        """`loss` on mu-law codes q.  input_codes (device int32
        [batch_size, T]): what the network reads in place of q, which stays
        the target of every row (input_noise.InputNoise.codes makes such
        codes); without it nothing but q is used, as ever."""
        self._refuse_mixture_codes('loss_from_codes')
        if input_codes is not None:
            self._refuse_scalar_noise('loss', 'input_codes')
        self._check_supported()
        q = q.reshape(self.batch_size, -1)
        q_in = self._check_input_codes(input_codes, q, 'loss')
        mask = check_lengths(lengths, loss_denominator, self.batch_size,
                             q.shape[1], 'loss')
        mask, hist = check_history(history, mask, loss_denominator,
                                   self.batch_size, q.shape[1], 'loss')
        lc = lcond.check(self, local_condition_batch, local_condition_offset,
                         self.batch_size, q.shape[1], 'loss')
        return self._loss(q, global_condition_batch,
                          l2_regularization_strength, backward, audio, lc,
                          mask, hist, q_in)

    # ---- inputs that differ from the targets (wavenet/input_noise.py)
    def _check_noise(self, input_noise, noise_keys, what):
        if (input_noise is None) != (noise_keys is None):
            raise ValueError('%s: input_noise and noise_keys go together'
                             % what)
        if input_noise is None:
            return
        if self.mol_K:
            raise ValueError('%s: input_noise is not for a mixture-of-'
                             'logistics model: its inputs are float audio on '
                             'the 16-bit grid, not codes' % what)
        from .input_noise import InputNoise
        if not isinstance(input_noise, InputNoise):
            raise ValueError('%s: input_noise must be an InputNoise, got %r'
                             % (what, input_noise))
        self._refuse_scalar_noise(what, 'input_noise')

    def _refuse_scalar_noise(self, what, name):
        if self.scalar_input:
            raise ValueError(
                '%s: %s is not for scalar_input models: their network input '
                'is the float audio, not the codes' % (what, name))

    def _refuse_mixture_codes(self, what):
        if self.mol_K:
            raise ValueError(
                '%s: a mixture-of-logistics model (output_mixture=%d) has no '
                'mu-law codes: its inputs and targets are the 65536 levels '
                'of the float audio; use loss / score / predict_mixture'
                % (what, self.mol_K))

    def _check_input_codes(self, input_codes, q, what):
        """input_codes as device int32 [B, T] beside codes q [B, T], or
        None."""
        if input_codes is None:
            return None
        if not isinstance(input_codes, torch.Tensor) or \
                input_codes.dtype != torch.int32 or \
                input_codes.device != self.device or \
                tuple(input_codes.shape) != tuple(q.shape):
            raise ValueError(
                '%s: input_codes must be an int32 tensor of shape %s on %s'
                % (what, tuple(q.shape), self.device))
        return input_codes

    def _encode_noisy(self, a, noise, keys, mask, training):
        """(q, q_in) of audio a [B, T] by the fused kernel, written straight
        into the workspace's q_tgt and q (what _loss and scoring.score would
        copy them into)."""
        B, T = a.shape
        ws = self._workspace(B, T, training)
        return noise.encode(a, self.Q, keys,
                            None if mask is None else mask[0],
                            out=(ws.q_tgt.view(B, T), ws.q.view(B, T)))

    def _loss(self, q, global_condition_batch, l2_regularization_strength,
              backward, audio, lc, mask=None, hist=None, q_in=None):
        """loss_from_codes on codes q [B, T] with the LC input checked
        (local_condition.check), the lengths (check_lengths) and the history
        (check_history).  q_in: what the network reads instead (q stays the
        target), or None."""
        B, T = q.shape
        N = B * T
        ws = self._workspace(B, T, backward)
        if backward and self._tail_work is not None:
            # the previous backward pass started its tail all-reduce and no
            # optimizer.minimize joined it: join before this pass rewrites the
            # bucket (parallel.begin_tail_allreduce documents why this keeps
            # the ranks in step)
            import warnings
            from . import parallel
            warnings.warn('the tail all-reduce of the previous backward pass '
                          'was never joined (no optimizer.minimize followed): '
                          'joined and dropped now')
            parallel.abandon_tail_allreduce(self)
        if self.mol_K:
            # (loss() quantised straight into ws.q and ws.audio: mol.stage)
            q_lab = ws.q
        else:
            q_lab = train_pass.stage_codes(ws, q, q_in)
        if self.scalar_input and not self.mol_K:
            # network input is the raw float audio (model.py:645-648)
            if audio is None:
                raise ValueError('scalar_input needs the float audio')
            ws.audio.copy_(audio.reshape(-1))
        ids = self._gc_ids(global_condition_batch, B)
        st = _lib.stream()
        lcond.fill(self, lc, ws)
        # (L2 adds lambda * params to the WHOLE bucket after the backward
        # pass: the tail must not have been summed over ranks before that)
        path = train_pass.step_path(
            self, ws, backward, l2=l2_regularization_strength is not None)
        train_pass.run_pass(self, 'fwd', ws, ids, path)
        quirk = 1 if self.tf_xent_zero_label_quirk else 0
        if self.mol_K:
            # one entry for plain, masked and windowed (null pointers: plain)
            den = float(N)
            if mask is not None:
                lengths, den = mask
                inv = np.float32(1.0) / np.float32(den)
                ws.xent_mask.copy_(torch.from_numpy(np.concatenate(
                    [lengths, np.array([inv], np.float32).view(np.int32)])))
                if hist is not None:
                    ws.xent_hist.copy_(torch.from_numpy(hist))
            mol.loss(self, ws, mask is not None, hist is not None, backward)
        elif mask is None:
            den = float(N)
            _lib.call('wn_xent', _lib.ptr(ws.logits), self.Q, _lib.ptr(q_lab),
                      _lib.ptr(ws.logits) if backward else None,
                      _lib.ptr(ws.loss_parts[2:]), B, T, self.Q, quirk, st)
        else:
            # the kernel scales by float32 1 / den as wn_xent does by 1 / N
            lengths, den = mask
            inv = np.float32(1.0) / np.float32(den)
            ws.xent_mask.copy_(torch.from_numpy(np.concatenate(
                [lengths, np.array([inv], np.float32).view(np.int32)])))
            if hist is None:
                _lib.call('wn_xent_masked', _lib.ptr(ws.logits), self.Q,
                          _lib.ptr(q_lab), _lib.ptr(ws.xent_mask),
                          _lib.ptr(ws.xent_mask[B:]),
                          _lib.ptr(ws.logits) if backward else None,
                          _lib.ptr(ws.loss_parts[2:]), B, T, self.Q, quirk,
                          st)
            else:
                # staged like the lengths: read by the kernel when it runs
                ws.xent_hist.copy_(torch.from_numpy(hist))
                _lib.call('wn_xent_window', _lib.ptr(ws.logits), self.Q,
                          _lib.ptr(q_lab), _lib.ptr(ws.xent_hist),
                          _lib.ptr(ws.xent_mask), _lib.ptr(ws.xent_mask[B:]),
                          _lib.ptr(ws.logits) if backward else None,
                          _lib.ptr(ws.loss_parts[2:]), B, T, self.Q, quirk,
                          st)
        _lib.call('wn_reduce_slabs', _lib.ptr(ws.loss_parts), ws.nparts + 2, 1, 1,
                  0, 0, 1, _lib.ptr(ws.loss), 0, 1, 0, st)
        loss = ws.loss[0] / den                         # reduce_mean, :666
        if backward:
            try:
                train_pass.run_pass(self, 'bwd', ws, ids, path)
            except BaseException:
                # (a launch error after the tail's all-reduce was issued: join
                # it, so that the next step does not find it dangling)
                from . import parallel
                parallel.abandon_tail_allreduce(self)
                raise
            # the backward stack launch's poison word (0, or NaN when one of
            # its dependency waits expired) is written after the loss
            # reduction above: add it here so that THIS step's loss is NaN
            # before the optimizer applies the step
            loss = loss + ws.loss_parts[1]
        if l2_regularization_strength is not None:
            lam = float(l2_regularization_strength)
            mask = None if self.tf_bias_name_quirk else self._l2_mask()
            _lib.call('wn_l2_partials', _lib.ptr(self.params),
                      self.params.numel(), _lib.ptr(mask),
                      _lib.ptr(ws.l2_parts) if backward else
                      _lib.ptr(self._l2_tmp()), st)
            parts = ws.l2_parts if backward else self._l2_tmp()
            loss = loss + lam * parts.sum()             # model.py:674-680
            if backward:
                _lib.call('wn_axpy', _lib.ptr(self.grads),
                          _lib.ptr(self.params), lam, _lib.ptr(mask),
                          self.params.numel(), st)
        loss._wn_model = self
        loss._wn_has_grads = bool(backward)
        return loss

    def score(self, input_batch, global_condition_batch=None, *,
              local_condition_batch=None, local_condition_offset=0,
              lengths=None, per_sample=False, history=None,
              input_noise=None, noise_keys=None):
        '''Scores held-out audio: per-clip negative log-likelihood, target
        count and top-1 hits.  Forward only -- the pass predict_proba makes,
        on the forward-only workspace: no gradient is touched, no all-reduce
        starts -- and without any host synchronisation.

        Inputs, their checks and their errors are those of `loss`
        (global_condition_batch, local_condition_batch / _offset, lengths),
        except that a 2-D input_batch [B, T] may have ANY number of rows
        B >= 1 (a validation set ends in a ragged batch); anything else is
        reshaped to [batch_size, -1].

        Returns scoring.Score(nll, count, correct, per_sample), device
        tensors: nll float64 [B], the sum over clip b's rows with a target
        of logsumexp(logits[b, t]) - logits[b, t, q[b, t + 1]] (nats);
        count int32 [B], the rows with a target (lengths[b] - 1, T - 1
        without lengths); correct int32 [B], those whose arg-max is the
        target; per_sample float32 [B, T], each row's term (0 where there is
        no target: the last real row and the padding), or None unless
        per_sample=True.

        Relation to the loss: loss(backward=False, lengths=n) ==
        nll.sum() / sum(n) and loss(backward=False) == nll.sum() / (B * T)
        (the reference's mean keeps the label-less rows in its denominator),
        while nll.sum() / count.sum() is the true mean negative
        log-likelihood per predicted sample, in nats; / ln 2 gives bits.

        history (as for `loss`): rows with t + 1 < history[b] have no target
        either: count[b] = n[b] - max(history[b], 1), and
        loss(backward=False, lengths=n, history=h) == nll.sum() /
        sum(n - h).

        input_noise, noise_keys (as for `loss`, one key per row of the
        batch): the network reads perturbed codes, the scored targets stay
        clean.

        A mixture-of-logistics model (output_mixture=K) is scored on the
        65536 levels: nll is the sum of -log P(level j[t + 1]) under the
        mixture, the relations above hold, and correct is None (an arg-max
        is not defined for this head).'''
        self._check_noise(input_noise, noise_keys, 'score')
        self._check_supported()
        a = input_batch
        if not isinstance(a, torch.Tensor):
            a = torch.as_tensor(np.asarray(a), dtype=torch.float32)
        B = a.shape[0] if a.dim() == 2 and a.shape[0] >= 1 \
            else self.batch_size
        a = a.to(device=self.device, dtype=torch.float32).reshape(B, -1)
        mask = check_lengths(lengths, None, B, a.shape[1], 'score')
        mask, hist = check_history(history, mask, None, B, a.shape[1],
                                   'score')
        lc = lcond.check(self, local_condition_batch, local_condition_offset,
                         B, a.shape[1], 'score')
        from . import scoring
        if self.mol_K:
            ws = self._workspace(B, a.shape[1], False)
            mol.stage(self, ws, a, mask)
            return scoring.score(self, ws.q.view(B, -1),
                                 global_condition_batch, ws.audio, lc, mask,
                                 per_sample, hist)
        if input_noise is None:
            q, q_in = mu_law_encode(a, self.Q), None
        else:
            q, q_in = self._encode_noisy(a, input_noise, noise_keys, mask,
                                         False)
        return scoring.score(self, q, global_condition_batch, a, lc, mask,
                             per_sample, hist, q_in)

    def score_from_codes(self, q, global_condition_batch=None, audio=None, *,
                         local_condition_batch=None, local_condition_offset=0,
                         lengths=None, per_sample=False, history=None,
                         input_codes=None):
        """`score` on mu-law codes q (int, [B, T] with any B >= 1, else
        reshaped to [batch_size, -1]); audio: the float audio a scalar_input
        model needs; input_codes (device int32, q's shape): what the network
        reads in place of q, which stays the target."""
        self._refuse_mixture_codes('score_from_codes')
        if input_codes is not None:
            self._refuse_scalar_noise('score', 'input_codes')
        self._check_supported()
        if not isinstance(q, torch.Tensor):
            q = torch.as_tensor(np.asarray(q))
        B = q.shape[0] if q.dim() == 2 and q.shape[0] >= 1 \
            else self.batch_size
        q = q.reshape(B, -1)
        q_in = self._check_input_codes(input_codes, q, 'score')
        mask = check_lengths(lengths, None, B, q.shape[1], 'score')
        mask, hist = check_history(history, mask, None, B, q.shape[1],
                                   'score')
        lc = lcond.check(self, local_condition_batch, local_condition_offset,
                         B, q.shape[1], 'score')
        from . import scoring
        return scoring.score(self, q, global_condition_batch, audio, lc, mask,
                             per_sample, hist, q_in)

    def _l2_tmp(self):
        if not hasattr(self, '_l2_parts'):
            self._l2_parts = torch.empty(_lib.load().wn_l2_partials_count(),
                                         dtype=torch.float32,
                                         device=self.device)
        return self._l2_parts

    def _l2_mask(self):
        """1 for weights, 0 for biases (only used when the TF bias-name quirk
        is switched off)."""
        if not hasattr(self, '_l2m'):
            m = torch.ones_like(self.params)
            tree = self._views(m)
            for n, v in self.named_variables(tree):
                if 'bias' in n.split('/')[-1]:
                    v.zero_()
            self._l2m = m
        return self._l2m

    def predict_proba(self, waveform, global_condition=None, name='wavenet',
                      *, local_condition=None):
        '''Computes the probability distribution of the next sample based on
        all samples in the input waveform (model.py:564-590).  waveform:
        already-quantised int samples.

        local_condition (LC models only, required there): float [B, T, Lc]
        (or [T, Lc] with batch_size 1), row t beside waveform sample t.  The
        returned distribution is that of the sample after the last one, so
        the last row conditions it.'''
        if self.mol_K:
            raise ValueError('predict_proba: a mixture-of-logistics model '
                             'has no probability vector over codes; use '
                             'predict_mixture')
        self._check_supported()
        B = self.batch_size
        w = waveform
        if not isinstance(w, torch.Tensor):
            w = torch.as_tensor(np.asarray(w))
        w = w.to(device=self.device, dtype=torch.int32).reshape(B, -1)
        T = w.shape[1]
        lc = lcond.rows(self, local_condition, B, T, 'predict_proba')
        ws = self._workspace(B, T, False)
        ws.q.copy_(w.reshape(-1))
        if self.scalar_input:
            # decode the codes back to floats in [-1, 1] (model.py:570-576)
            ws.audio.copy_(mu_law_decode(w, self.Q).reshape(-1))
        ids = self._gc_ids(global_condition, B)
        lcond.fill(self, lc, ws)
        train_pass.run_pass(self, 'fwd', ws, ids,
                            train_pass.step_path(self, ws, False))
        out = torch.empty(self.Q, dtype=torch.float32, device=self.device)
        _lib.call('wn_softmax64_row', _lib.ptr(ws.logits[B * T - 1]), self.Q,
                  _lib.ptr(out), _lib.stream())
        # 0, or NaN when a dependency wait of the forward stack launch
        # expired: wrong probabilities are never returned silently
        return out + ws.loss_parts[0]

    def predict_mixture(self, audio_so_far, global_condition=None, *,
                        local_condition=None):
        '''The mixture of the next sample given all samples so far: the
        counterpart of predict_proba for a model built with
        output_mixture=K.  audio_so_far: float samples, anything reshapeable
        to [batch_size, -1]; they are snapped to the 65536 levels and the
        network reads the centres, as in training.  local_condition: as
        predict_proba's.  Returns device float32 [3, K] of the last row of
        the last clip: log_softmax(pi), mu and the clamped beta
        (wn_mol_params_row), which mol.sample draws from.'''
        if not self.mol_K:
            raise ValueError('predict_mixture: this model was built without '
                             'output_mixture; use predict_proba')
        self._check_supported()
        B = self.batch_size
        a = audio_so_far
        if not isinstance(a, torch.Tensor):
            a = torch.as_tensor(np.asarray(a), dtype=torch.float32)
        a = a.to(device=self.device, dtype=torch.float32).reshape(B, -1)
        T = a.shape[1]
        lc = lcond.rows(self, local_condition, B, T, 'predict_mixture')
        ws = self._workspace(B, T, False)
        mol.stage(self, ws, a, None)
        ids = self._gc_ids(global_condition, B)
        lcond.fill(self, lc, ws)
        train_pass.run_pass(self, 'fwd', ws, ids,
                            train_pass.step_path(self, ws, False))
        # 0, or NaN when a dependency wait of the forward stack launch
        # expired (as predict_proba)
        return mol.params_row(self, ws.logits[B * T - 1]) + ws.loss_parts[0]

    # ------------------------------------------ fast generation (fastgen.py)
    FASTGEN_MAX_CHANNELS = 1024    # wn_fastgen_run_wide (FGW_MAXC)
    FASTGEN_BATCH_MAX = 256        # wn_fastgen_batch_* (FGB_MAXB)

    def predict_proba_incremental(self, waveform, global_condition=None,
                                  name='wavenet', push=True, *,
                                  local_condition=None):
        '''Computes the probability distribution of the next sample
        incrementally, based on a single sample and all previously passed
        samples (model.py:592-626).  Eager counterpart of running the
        reference's proba op together with `net.push_ops` (push=True) or
        alone (push=False); `net.reset_generator()` is `net.init_ops`.

        local_condition (LC models only, required there): float [Lc] or
        [1, Lc], the row beside the sample pushed or peeked.  An LC model's
        generator is reset with prime_generator([], local_condition=
        np.zeros((0, Lc))).'''
        lc = local_condition
        if self.Lc and lc is not None and np.ndim(lc) == 1:
            lc = lc.reshape(1, -1) if isinstance(lc, torch.Tensor) \
                else np.asarray(lc).reshape(1, -1)
        lc = lcond.fastgen_rows(self, lc, 'predict_proba_incremental', 1)
        return fastgen.predict_proba_incremental(self, waveform,
                                                 global_condition, push, lc)

    def reset_generator(self):
        """net.init_ops: refill every queue with zeros (model.py:457-479).
        An LC model refuses it: its generator is reset with
        prime_generator([], local_condition=np.zeros((0, Lc)))."""
        lcond.refuse_fastgen(self, 'reset_generator')
        fastgen.generator(self, None)
        fastgen.reset(self)

    def generate(self, num_samples, seed_samples=None, temperature=1.0,
                 global_condition=None, seed=0, return_proba_every=0, *,
                 local_condition=None, top_k=None, top_p=None):
        """The whole generate.py:195-241 loop on the device: prime with
        `seed_samples` (int codes; default one random-free seed 128 as in
        test_model.py:63), then draw `num_samples` samples with temperature.
        Returns int32 codes [len(seed) + num_samples] (and the probabilities
        of every `return_proba_every`-th step when requested).

        local_condition (LC models only, required there): float
        [len(seed) + num_samples - 1, Lc], row i beside code i of the result
        (it conditions the prediction of code i + 1).  The generator is
        reset internally (reset_generator itself refuses LC models).

        top_k, top_p: truncate every draw to the top_k most probable codes
        and / or the top_p nucleus of the tempered distribution (the rule:
        wavenet/sampling.py).  Per call, not remembered; None, top_k >= Q and
        top_p == 1 draw from all codes.  The returned probabilities stay the
        untruncated softmax."""
        sampling.check(top_k, top_p)
        lc = None
        if self.Lc or local_condition is not None:
            lc = lcond.fastgen_rows(self, local_condition, 'generate',
                                    _n_codes(seed_samples) + int(num_samples)
                                    - 1)
        return fastgen.generate(self, num_samples, seed_samples, temperature,
                                global_condition, seed, return_proba_every,
                                lc, top_k, top_p)

    def prime_generator(self, codes, global_condition=None, *,
                        local_condition=None):
        """Set the incremental-generation queues to the state they have after
        `codes` were pushed one by one from a fresh `reset_generator()`, using
        ONE batch forward pass: layer l's queue (capacity d_l) holds the last
        d_l inputs x_l[t] of that layer (model.py:473-484), which are rows of
        the forward pass's per-layer activation planes.

        local_condition (LC models only, required there): float
        [len(codes), Lc], row i beside codes[i]; with no codes and
        np.zeros((0, Lc)) this resets an LC model's generator."""
        lc = lcond.fastgen_rows(self, local_condition, 'prime_generator',
                                _n_codes(codes))
        if lc is not None and lc.shape[0] > 0 and \
                not lcond.forward_ok(self, lc.shape[0]):
            raise NotImplementedError(
                'prime_generator: the forward pass that primes an LC model '
                'is the persistent stack launch (wn_stack_fwd_lc): '
                + self.LC_SUPPORTED + ', fewer than 2^24 codes')
        fastgen.prime(self, codes, global_condition, lc)

    def continue_generation(self, num_samples, last_sample, temperature=1.0,
                            global_condition=None, seed=0, *,
                            local_condition=None, top_k=None, top_p=None):
        """Draw `num_samples` more samples after `generate` (the queues stay
        on the device; `last_sample` is the last code drawn so far, which has
        not been pushed yet).  Returns the new int32 codes.

        local_condition (LC models only, required there): float
        [num_samples, Lc]; row 0 sits beside `last_sample`, row k beside new
        code k - 1.  generate(a) then continue_generation(b) on consecutive
        rows is the process of one generate(a + b).

        top_k, top_p: as generate's, for this call only (a truncated
        generate does not make its continuation truncated)."""
        sampling.check(top_k, top_p)
        lc = lcond.fastgen_rows(self, local_condition, 'continue_generation',
                                int(num_samples))
        return fastgen.continue_generation(self, num_samples, last_sample,
                                           temperature, global_condition, seed,
                                           lc, top_k, top_p)

    def generate_batch(self, num_samples, seeds, seed_samples=None,
                       temperature=1.0, global_condition=None,
                       return_proba_every=0, *, local_condition=None,
                       top_k=None, top_p=None, reserve_steps=None):
        """`generate` for B = len(seeds) independent streams stepped in lock
        step (1 <= B <= 256).  Stream b draws with seeds[b] under generate()'s
        counter rule, so it is the same random process as
        generate(seed=seeds[b]), and its results do not depend on the other
        streams.  seed_samples: None (Q // 2 for every stream), one sequence
        shared by all streams, or [B, n]; global_condition: None, one id, or
        B ids.  Returns int32 [B, n + num_samples] (and float32
        [B, ceil(steps / k), Q] probabilities with return_proba_every = k).

        local_condition (LC models only, required there): float
        [B, n + num_samples - 1, Lc] (n seed codes per stream), or
        [n + num_samples - 1, Lc] shared by all streams; rows as generate's.

        top_k, top_p: as generate's; one setting for all streams.

        reserve_steps: the longest call (in steps) of the run this call
        starts; buffers are sized for it once, so that this call and its
        continuations (given the same value) share their captured graphs."""
        sampling.check(top_k, top_p)
        # (the rows are checked in _batch_args's order, beside the seed codes)
        if self.Lc and local_condition is None:
            lcond.refuse_fastgen(self, 'generate_batch')
        return fastgen.generate_batch(self, num_samples, seeds, seed_samples,
                                      temperature, global_condition,
                                      return_proba_every, local_condition,
                                      top_k, top_p, reserve_steps)

    def continue_generation_batch(self, num_samples, last_samples, seeds,
                                  temperature=1.0, global_condition=None,
                                  return_proba_every=0, *,
                                  local_condition=None, top_k=None,
                                  top_p=None, restart=None,
                                  reserve_steps=None):
        """Draw `num_samples` more samples for every stream of the last
        generate_batch call (the queues stay on the device; last_samples[b]
        is stream b's last code so far, not yet pushed).  Returns int32
        [B, num_samples] (and the probabilities, as generate_batch).

        local_condition (LC models only, required there): float
        [B, num_samples, Lc] or [num_samples, Lc], rows as
        continue_generation's.

        top_k, top_p: as generate's, for this call only.

        restart: None, or stream indices (ints in [0, B), no duplicates).
        Those streams start over with this call: stream b's result is, bit
        for bit, generate_batch(num_samples, [seeds[b]], seed_samples=
        [[last_samples[b]]], global_condition=gc[b], local_condition=
        lc[b:b + 1])[0, 1:] run alone (zero queues, no previous code, the
        draw counted from this call's first step); later calls without
        restart continue that process.  The other streams are unaffected.

        reserve_steps: as generate_batch's."""
        sampling.check(top_k, top_p)
        if self.Lc and local_condition is None:
            lcond.refuse_fastgen(self, 'continue_generation_batch')
        return fastgen.continue_generation_batch(
            self, num_samples, last_samples, seeds, temperature,
            global_condition, return_proba_every, local_condition, top_k,
            top_p, restart, reserve_steps)

    # ---- mixture-of-logistics models (output_mixture=K): the batched
    # generator on levels (csrc/wn_fastgen_mol.hip)
    def generate_mixture_batch(self, num_samples, seeds, seed_levels=None,
                               temperature=1.0, global_condition=None,
                               return_params_every=0, *, local_condition=None,
                               reserve_steps=None):
        """`generate_batch` for a model built with output_mixture=K: B =
        len(seeds) independent streams in lock step (1 <= B <= 256), each
        drawing 16-bit levels from its mixture as mol.sample does, with
        seeds[b] and counter = the stream's step (the seed's steps count).
        seed_levels: None (level 32768 for every stream), one sequence of
        levels (ints in 0 .. 65535) shared by all streams, or [B, n];
        temperature >= 0 (0: the mean of the drawn component).  Returns int32
        levels [B, n + num_samples]; with return_params_every = k also
        float32 [B, ceil(steps / k), 3, K], the format of predict_mixture
        (log_softmax(pi), mu, clamped beta) of every k-th step.  A stream's
        levels and parameter bits do not depend on the other streams.

        global_condition, local_condition, reserve_steps: as generate_batch's.
        Limits: at most 32 residual / dilation channels, filter_width 2,
        initial_filter_width 1 .. 32, skip_channels <= 512, 64 layers."""
        if self.Lc and local_condition is None and self.mol_K:
            lcond.refuse_fastgen(self, 'generate_mixture_batch')
        return fastgen.generate_mixture_batch(
            self, num_samples, seeds, seed_levels, temperature,
            global_condition, return_params_every, local_condition,
            reserve_steps)

    def continue_mixture_batch(self, num_samples, last_levels, seeds,
                               temperature=1.0, global_condition=None,
                               return_params_every=0, *, local_condition=None,
                               restart=None, reserve_steps=None):
        """Draw `num_samples` more levels for every stream of the last
        generate_mixture_batch call, as continue_generation_batch does for
        codes: last_levels[b] is stream b's last level so far, not yet
        pushed.  Returns int32 [B, num_samples] (and the parameters, as
        generate_mixture_batch).  restart: stream indices that start over
        with this call (empty history, zero queues, the draw counted from
        this call's first step); bit for bit a fresh stream from there on."""
        if self.Lc and local_condition is None and self.mol_K:
            lcond.refuse_fastgen(self, 'continue_mixture_batch')
        return fastgen.continue_mixture_batch(
            self, num_samples, last_levels, seeds, temperature,
            global_condition, return_params_every, local_condition, restart,
            reserve_steps)

    def generate_mixture(self, num_samples, seed_levels=None, temperature=1.0,
                         global_condition=None, seed=0,
                         return_params_every=0, *, local_condition=None,
                         reserve_steps=None):
        """generate_mixture_batch with one stream, squeezed: int32 levels
        [n + num_samples] (and float32 [rows, 3, K]).  It runs on the batched
        generator's state (there is no single-stream kernel for levels), so a
        generate_mixture_batch call in between starts that state over."""
        lc = local_condition
        if lc is not None and np.ndim(lc) == 2:
            lc = lc[None]
        out = self.generate_mixture_batch(
            num_samples, [seed], seed_levels, temperature, global_condition,
            return_params_every, local_condition=lc,
            reserve_steps=reserve_steps)
        return (out[0][0], out[1][0]) if isinstance(out, tuple) else out[0]

    def continue_mixture(self, num_samples, last_level, temperature=1.0,
                         global_condition=None, seed=0,
                         return_params_every=0, *, local_condition=None,
                         reserve_steps=None):
        """continue_mixture_batch with one stream, squeezed; it continues
        the batched generator's state that generate_mixture left."""
        lc = local_condition
        if lc is not None and np.ndim(lc) == 2:
            lc = lc[None]
        out = self.continue_mixture_batch(
            num_samples, [int(last_level)], [seed], temperature,
            global_condition, return_params_every, local_condition=lc,
            reserve_steps=reserve_steps)
        return (out[0][0], out[1][0]) if isinstance(out, tuple) else out[0]

    def batch_local_condition(self, items, position, num_steps):
        """The local_condition rows [B, num_steps, Lc] (device float32) of a
        continue_generation_batch call whose first step is lock-step step
        `position`, for streams that hold different items: items[b] is
        None (zero rows) or (rows, origin), rows a contiguous float32 device
        tensor [m, Lc] and origin the step at which stream b (re)started.
        The stream's own step t = position + j - origin gets rows[t - 1] for
        1 <= t <= m and zeros elsewhere (step 0 sits beside the given first
        code).  One launch, no host wait."""
        if not self.Lc:
            raise ValueError('batch_local_condition: this model was built '
                             'without local conditioning')
        return fastgen.batch_lc_rows(self, items, position, num_steps)
