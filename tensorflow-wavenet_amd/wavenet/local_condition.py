"""Local conditioning (LC, WaveNet paper 2.5), host side: the constructor's
LC keywords, the one check of a call's LC input, the front end that fills the
rows `ws.lc`, the LC gradients and workspace buffers, the CLIs' LC flags.
Functions take the model first; the limits are WaveNetModel.LC_*."""
import collections
import ctypes
import types

import numpy as np
import torch

from . import _lib
from . import train_pass

# a checked frames input: frames [B, F, Lc] (a float tensor where the caller
# had them), offsets int64 [B], clip length T, the staging window (window)
Frames = collections.namedtuple('Frames', 'frames off T idx inside')


def _align4(n):
    return (n + 3) // 4 * 4


def configure(net, lc, scales, p):
    """Check the LC keywords (before any library or device is touched) and
    set Lc (0: no LC), Lcp (padded to 4), the upsampler's scales lc_up and
    hop (None / 0: rows at audio rate) and the context half-width lc_ctx."""
    net.local_condition_channels = lc
    net.Lc, net.lc_up, net.lc_hop, net.lc_ctx = 0, None, 0, None
    if lc is not None:
        if isinstance(lc, bool) or int(lc) != lc or int(lc) <= 0:
            raise ValueError('local_condition_channels must be a positive '
                             'int, got %r' % (lc,))
        why = None
        if max(int(net.residual_channels), int(net.dilation_channels)) > 32:
            why = 'more than 32 residual / dilation channels'
        elif int(net.filter_width) != 2:
            why = 'filter_width %d' % int(net.filter_width)
        elif net.scalar_input and not getattr(net, 'mol_K', 0):
            # (a mixture-of-logistics model reads scalar input and carries
            # LC: the LC arithmetic lives in the stack launches, the scalar
            # causal layer is a launch of its own)
            why = 'scalar_input without output_mixture'
        if why:
            raise NotImplementedError('%s: %s' % (why, net.LC_SUPPORTED))
        net.Lc = int(lc)
    net.Lcp = _align4(net.Lc)
    if scales is not None:
        if lc is None:
            raise ValueError('local_condition_upsample_scales needs '
                             'local_condition_channels')
        try:
            sc = tuple(scales)
        except TypeError:
            raise ValueError('local_condition_upsample_scales must be a tuple '
                             'of ints, got %r' % (scales,))
        if not 1 <= len(sc) <= net.LC_UPSAMPLE_MAX_LAYERS or any(
                isinstance(s, (bool, np.bool_)) or
                not isinstance(s, (int, np.integer)) or int(s) < 2
                for s in sc):
            raise ValueError('local_condition_upsample_scales must be 1 to %d '
                             'ints >= 2, got %r'
                             % (net.LC_UPSAMPLE_MAX_LAYERS, scales))
        net.lc_up = tuple(int(s) for s in sc)
        net.lc_hop = int(np.prod(net.lc_up))
        if net.lc_hop > net.LC_UPSAMPLE_MAX_HOP:
            raise ValueError('local_condition_upsample_scales: the hop (their '
                             'product, %d) must be at most %d'
                             % (net.lc_hop, net.LC_UPSAMPLE_MAX_HOP))
        if int(lc) > net.LC_UPSAMPLE_MAX_CHANNELS:
            raise NotImplementedError(
                'the local-conditioning upsampler supports at most %d '
                'channels (local_condition_channels = %d)'
                % (net.LC_UPSAMPLE_MAX_CHANNELS, int(lc)))
    # (the scales as the host int array the upsampler launches read; kept
    # alive with the model, recorded launch plans hold its address)
    net._lc_up_c = (ctypes.c_int * len(net.lc_up))(*net.lc_up) \
        if net.lc_up else None
    if p is not None:
        if isinstance(p, (bool, np.bool_)) or \
                not isinstance(p, (int, np.integer)) or \
                not 0 <= int(p) <= net.LC_CONTEXT_MAX:
            raise ValueError('local_condition_context must be an int from 0 '
                             'to %d, got %r' % (net.LC_CONTEXT_MAX, p))
        if not net.lc_up:
            raise ValueError('local_condition_context needs '
                             'local_condition_upsample_scales (it convolves '
                             'frames; repetition-row models take rows)')
        net.lc_ctx = int(p)
    net.local_condition_upsample_scales = net.lc_up
    net.local_condition_context = net.lc_ctx


def up_floats(net):
    """Floats of the upsampler's weights (bucket segment lc_up)."""
    return 3 * sum(net.lc_up) + (len(net.lc_up) if net.use_biases else 0)


def frame_window(net, T):
    """Frames a clip of T samples touches at most (any offset)."""
    return (T + net.lc_hop - 2) // net.lc_hop + 1


def launch_checks(net, N):
    """The 32-row stack launches, the only ones LC runs, cover N rows."""
    if not (net.stack_fwd and net.stack_bwd):
        raise NotImplementedError(
            'stack_fwd / stack_bwd = False with local conditioning: '
            + net.LC_SUPPORTED)
    if net._layer_path() != 'layer':       # (generic_layers forced)
        raise NotImplementedError(net.LC_SUPPORTED)
    if not net._stack_ok(N):
        raise NotImplementedError(
            'local conditioning needs B * T < 2^24 and at most 256 '
            'layers (the persistent stack launches)')


def forward_ok(net, n0):
    """The forward pass over n0 seed codes (forward priming) carries the LC
    rows (wn_stack_fwd_lc); otherwise the seed is stepped through."""
    return bool(net.stack_fwd and net.stack_bwd and net._stack_ok(n0))


def _plain(net, lc, what):
    """True for a model without LC, which refuses rows."""
    if net.Lc:
        return False
    if lc is not None:
        raise ValueError('%s: this model was built without local '
                         'conditioning (local_condition_channels=None)'
                         % what)
    return True


def _tensor(lc, what, dtype=None):
    """LC rows as a tensor where the caller had them (host: as `dtype`)."""
    if isinstance(lc, torch.Tensor):
        return lc
    lc = np.asarray(lc, dtype=dtype)
    if lc.dtype == object:
        raise ValueError('%s: local_condition must be a float array' % what)
    return torch.from_numpy(lc)


def rows(net, lc, B, T, what):
    """A call's rows [B, T, Lc] (or [T, Lc] with B = 1) and their launches,
    checked: float32 on the device (None without LC)."""
    if _plain(net, lc, what):
        return None
    if lc is None:
        raise ValueError('%s: the model was built with local conditioning '
                         '(%d channels); an lc batch [%d, %d, %d] is required'
                         % (what, net.Lc, B, T, net.Lc))
    lc = _tensor(lc, what, np.float32)
    if B == 1 and lc.dim() == 2:
        lc = lc.unsqueeze(0)
    if tuple(lc.shape) != (B, T, net.Lc):
        raise ValueError('%s: local conditioning must have shape [B, T, Lc] '
                         '= [%d, %d, %d] (row t beside input sample t), got %s'
                         % (what, B, T, net.Lc, tuple(lc.shape)))
    if not lc.is_floating_point():
        raise ValueError('%s: local conditioning must be floating point'
                         % what)
    launch_checks(net, B * T)
    return lc.to(device=net.device, dtype=torch.float32)


def check(net, lc, offset, B, T, what):
    """A loss call's LC input, checked: rows, or (upsampler) Frames."""
    if not net.lc_up:
        if not (isinstance(offset, (int, np.integer)) and
                not isinstance(offset, bool) and int(offset) == 0):
            raise ValueError('%s: local_condition_offset is for models '
                             'built with local_condition_upsample_scales'
                             % what)
        return rows(net, lc, B, T, what)
    fr, off = frames(net, lc, offset, B, T, what)
    launch_checks(net, B * T)
    return Frames(fr, off, T, *window(net, off, fr.shape[1], T))


def frames(net, fr, offset, B, T, what):
    """Frame-rate LC features [B, F, Lc] (or [F, Lc] with B = 1) and the
    offsets (an int or B non-negative ints), checked: the frames as a float
    tensor where the caller had them, the offsets as int64 numpy [B]."""
    Lc, hop = net.Lc, net.lc_hop
    shape = '[B, F, Lc] = [%d, F, %d] with F >= (offset + %d - 1) // %d + 1' \
        % (B, Lc, T, hop)
    if fr is None:
        raise ValueError('%s: the model upsamples local conditioning '
                         '(hop %d); frames %s are required'
                         % (what, hop, shape))
    if not isinstance(fr, torch.Tensor):
        fr = np.asarray(fr)
        if fr.dtype == object or not np.issubdtype(fr.dtype, np.floating):
            raise ValueError('%s: local conditioning frames must be a '
                             'float array %s' % (what, shape))
        fr = torch.from_numpy(fr)
    if not fr.is_floating_point():
        raise ValueError('%s: local conditioning frames must be floating '
                         'point' % what)
    if B == 1 and fr.dim() == 2:
        fr = fr.unsqueeze(0)
    if fr.dim() != 3 or fr.shape[0] != B or fr.shape[2] != Lc or \
            fr.shape[1] < 1:
        raise ValueError('%s: local conditioning frames must have shape %s,'
                         ' got %s' % (what, shape, tuple(fr.shape)))
    if isinstance(offset, torch.Tensor):
        offset = offset.detach().cpu().numpy()
    off = np.asarray(offset)
    if off.dtype == object or off.dtype == np.bool_ or \
            not np.issubdtype(off.dtype, np.integer):
        raise ValueError('%s: local_condition_offset must be an int or %d '
                         'ints, got %r' % (what, B, offset))
    if off.ndim == 0:
        off = np.full(B, int(off), np.int64)
    if off.shape != (B,):
        raise ValueError('%s: local_condition_offset must be an int or %d '
                         'ints, got shape %s' % (what, B, off.shape))
    off = off.astype(np.int64)
    if (off < 0).any():
        raise ValueError('%s: local_condition_offset must be non-negative, '
                         'got %s' % (what, off.tolist()))
    need = int(((off + T - 1) // hop).max()) + 1
    if fr.shape[1] < need:
        raise ValueError('%s: %d frames do not cover position offset + T - '
                         '1 = %d: local conditioning frames must have shape '
                         '%s (here F >= %d), got %s'
                         % (what, fr.shape[1], int((off + T - 1).max()),
                            shape, need, tuple(fr.shape)))
    return fr, off


def window(net, off, F, T):
    """Frame indices [B][frame_window + 2p] from offset // hop - p on (p = 0
    without context) and whether each lies inside [0, F)."""
    p = net.lc_ctx or 0
    idx = (off // net.lc_hop - p)[:, None] + \
        np.arange(frame_window(net, T) + 2 * p)[None, :]
    return idx, (idx >= 0) & (idx < F)


def refuse_fastgen(net, what):
    """An LC model's fast entry points refuse to run without rows."""
    if net.Lc:
        raise NotImplementedError(
            '%s: an LC model generates fast with local_condition=... '
            '(one row per input position the call steps through), or '
            'naively with predict_proba(..., local_condition=...) '
            '(generate.py --fast_generation false)%s'
            % (what, '' if what != 'reset_generator' else
               "; reset an LC model's generator with prime_generator([], "
               'local_condition=np.zeros((0, Lc)))'))


def fastgen_rows(net, lc, what, T, B=None):
    """The fast entry points' LC rows, checked: None without LC; else a
    float tensor where the caller had them, [T, Lc] (B None) or
    [B or 1, T, Lc] (B streams: one set each, or one shared)."""
    if _plain(net, lc, what):
        return None
    if lc is None:
        refuse_fastgen(net, what)
    if net.S > 512 or net.Q > 512 or net.L > 64:
        raise NotImplementedError(
            '%s: fast generation with local conditioning supports at most '
            '512 skip / quantization channels and 64 layers (this model: '
            'S = %d, Q = %d, L = %d); use predict_proba'
            % (what, net.S, net.Q, net.L))
    lc = _tensor(lc, what)
    if not lc.is_floating_point():
        raise ValueError('%s: local_condition must be floating point'
                         % what)
    shape, Lc = tuple(lc.shape), net.Lc
    if B is None:
        if shape != (T, Lc):
            raise ValueError('%s: local_condition must have shape [%d, %d] '
                             '(one row per input position), got %s'
                             % (what, T, Lc, shape))
    elif shape == (T, Lc):
        lc = lc.unsqueeze(0)
    elif shape != (B, T, Lc):
        raise ValueError('%s: local_condition must have shape '
                         '[%d, %d, %d] or [%d, %d] (shared by all '
                         'streams), got %s'
                         % (what, B, T, Lc, T, Lc, shape))
    return lc


def fill(net, lc, buf):
    """buf.lc [B * T][Lcp] (buf: a workspace or upsample's buffers) = the
    rows of a checked LC value: rows copied, or Frames staged -> context
    convolution into buf.lc_frames -> upsampler."""
    if lc is None:
        return
    if not isinstance(lc, Frames):
        buf.lc[:, :net.Lc].copy_(lc.reshape(-1, net.Lc))
        return
    st, B, ctx = _lib.stream(), lc.frames.shape[0], net.lc_ctx
    stage(net, lc, buf.lc_frames if ctx is None else buf.lc_xframes,
           buf.lc_off)
    if ctx is not None:
        _lib.call('wn_lc_context_fwd', _lib.ptr(buf.lc_xframes),
                  buf.lc_xframes.shape[1],
                  _lib.ptr(net._seg(net.params, 'lc_ctx')), ctx, net.Lc,
                  _lib.ptr(buf.lc_frames), buf.lc_frames.shape[1], B, st)
    _lib.call('wn_lc_upsample_fwd', _lib.ptr(buf.lc_frames),
              buf.lc_frames.shape[1], _lib.ptr(buf.lc_off),
              _lib.ptr(net._seg(net.params, 'lc_up')),
              ctypes.addressof(net._lc_up_c), len(net.lc_up), net.Lc,
              1 if net.use_biases else 0, _lib.ptr(buf.lc), net.Lcp, B, lc.T,
              st)


def stage(net, lc, dst, dst_off):
    """The window's frames into dst [B][Fx][Lc] (device) and offset[b] % hop
    into dst_off.  Outside [0, F) a context model (p = 0 included) writes
    zero rows; a model without context clamps to frame F - 1."""
    fr = lc.frames
    B, F = fr.shape[0], fr.shape[1]
    rows_ = torch.arange(B, device=fr.device)[:, None]
    sel = fr[rows_, torch.as_tensor(np.clip(lc.idx, 0, F - 1),
                                    device=fr.device)]
    if net.lc_ctx is not None:
        keep = torch.as_tensor(lc.inside, device=fr.device)[:, :, None]
        sel = torch.where(keep, sel, torch.zeros((), dtype=sel.dtype,
                                                 device=sel.device))
    dst.copy_(sel)
    dst_off.copy_(torch.as_tensor((lc.off % net.lc_hop).astype(np.int32)))


def upsample(net, fr, num_samples, offset):
    """WaveNetModel.upsample_local_condition, on buffers of its own."""
    net._check_supported()
    if not net.lc_up:
        raise ValueError('upsample_local_condition: the model was built '
                         'without local_condition_upsample_scales')
    n = int(num_samples)
    if n < 1:
        raise ValueError('upsample_local_condition: num_samples must be '
                         'positive, got %r' % (num_samples,))
    if not isinstance(fr, torch.Tensor):
        fr = np.asarray(fr)
    two_d = fr.ndim == 2
    B = 1 if two_d or fr.ndim < 2 else fr.shape[0]
    fr, off = frames(net, fr, offset, B, n, 'upsample_local_condition')
    lc = Frames(fr, off, n, *window(net, off, fr.shape[1], n))
    f32 = dict(dtype=torch.float32, device=net.device)
    Fw, p = frame_window(net, n), net.lc_ctx
    buf = types.SimpleNamespace(
        lc=torch.empty((B * n, net.Lcp), **f32),
        lc_frames=torch.empty((B, Fw, net.Lc), **f32),
        lc_off=torch.empty((B,), dtype=torch.int32, device=net.device),
        lc_xframes=None if p is None else torch.empty(
            (B, Fw + 2 * p, net.Lc), **f32))
    fill(net, lc, buf)
    out = buf.lc[:, :net.Lc].reshape(B, n, net.Lc).contiguous()
    return out[0] if two_d else out


def backward(net, ws, st):
    """The LC gradients: d lc_w = lc^T lc_da (da_f | da_g the backward stack
    stored); d rows = lc_da lc_w^T, the upsampler's (layer, slot, tap)
    partials per workgroup summed in a fixed order; the context's from d ctx."""
    N, W64, Lcp = ws.N, net.L * 64, net.Lcp
    reg = ws.region['lc_w']
    _lib.call_timed('wn_gemm_tn', (
        _lib.ptr(ws.lc), Lcp, 0, 0, None, 0, ws.T, _lib.ptr(ws.lc_da), W64,
        _lib.ptr(reg.buf), reg.count, N, Lcp, W64, 0, st),
        2.0 * N * W64 * Lcp, net._gemm_events)
    train_pass.reduce_slabs(reg, _lib.ptr(net._seg(net.grads, 'lc_w')), st)
    if not net.lc_up:
        return
    _lib.call('wn_transpose', _lib.ptr(net._seg(net.params, 'lc_w')), Lcp,
              W64, W64, _lib.ptr(ws.lc_wT), Lcp, st)
    _lib.call_timed('wn_gemm_nn', (
        _lib.ptr(ws.lc_da), W64, 0, 0, _lib.ptr(ws.lc_wT), Lcp, None, None,
        0, None, 0, _lib.ptr(ws.lc_drows), Lcp, 0, 0, None, N, Lcp, W64, 0,
        st), 2.0 * N * W64 * Lcp, net._gemm_events)
    reg = ws.region['lc_up']
    args = (_lib.ptr(ws.lc_frames), ws.lc_fw, _lib.ptr(ws.lc_off),
            _lib.ptr(net._seg(net.params, 'lc_up')),
            ctypes.addressof(net._lc_up_c), len(net.lc_up), net.Lc,
            1 if net.use_biases else 0, _lib.ptr(ws.lc_drows), Lcp, ws.B,
            ws.T, _lib.ptr(reg.buf), reg.count, reg.stride)
    if net.lc_ctx is None:
        _lib.call('wn_lc_upsample_bwd', *args, st)
    else:
        # (the same slabs) + d ctx
        _lib.call('wn_lc_upsample_bwd_ctx', *args, _lib.ptr(ws.lc_dctx),
                  _lib.ptr(ws.lc_dpart), st)
    train_pass.reduce_slabs(reg, _lib.ptr(net._seg(net.grads, 'lc_up')), st)
    if net.lc_ctx is not None:
        # d W[k] = sum over frames of x[f + k]^T d ctx[f]
        reg = ws.region['lc_ctx']
        _lib.call('wn_lc_context_wgrad', _lib.ptr(ws.lc_xframes),
                  ws.lc_xframes.shape[1], _lib.ptr(ws.lc_dctx), ws.lc_fw,
                  net.lc_ctx, net.Lc, ws.B, _lib.ptr(reg.buf), reg.count,
                  reg.stride, st)
        train_pass.reduce_slabs(reg, _lib.ptr(net._seg(net.grads, 'lc_ctx')), st)


def alloc_workspace(net, ws, alloc, region):
    """Workspace ws's LC buffers: the forward ones (region None), or the
    backward ones and their slab regions (`region`: the workspace's call
    that declares one, workspace.py)."""
    if not net.Lc:
        return
    L, Lc, B, N = net.L, net.Lc, ws.B, ws.N
    lib = _lib.load()
    if region is None:
        # the rows and lc x lc_w [N][L][64] (filter | gate, wn_stack_fwd_lc)
        alloc('lc', (N, net.Lcp), fill=0.0)
        alloc('lc_add', (N, L * 64))
        if net.lc_up:
            # the staged frames [B][Fw][Lc] and the offsets in the first one
            ws.lc_fw = frame_window(net, ws.T)
            alloc('lc_frames', (B, ws.lc_fw, Lc), fill=0.0)
            alloc('lc_off', (B,), torch.int32, fill=0)
        if net.lc_ctx is not None:
            # context: staged [B][Fw + 2p][Lc]; lc_frames is its output
            alloc('lc_xframes', (B, ws.lc_fw + 2 * net.lc_ctx, Lc), fill=0.0)
        return
    # the pre-activation gradients [N][L][64] for lc^T da, whose TN GEMM's
    # slabs share ws.slabs
    alloc('lc_da', (N, L * 64))
    region('lc_w', lib.wn_gemm_tn_splits(N, net.Lcp, L * 64, 0),
           lib.wn_gemm_tn_slab_floats(net.Lcp, L * 64), net.Lcp * L * 64)
    if net.lc_up:
        # d rows = lc_da lc_w^T, the upsampler's per-workgroup slabs
        alloc('lc_wT', (L * 64, net.Lcp))
        alloc('lc_drows', (N, net.Lcp))
        n = up_floats(net)
        nslab = lib.wn_lc_upsample_bwd_slabs(N, n)
        region('lc_up', nslab, _align4(n), n, own='lc_up_slabs')
    if net.lc_ctx is not None:
        # d ctx [B][Fw][Lc], workgroups' parts of shared frames, slabs
        alloc('lc_dctx', (B, ws.lc_fw, Lc))
        alloc('lc_dpart', (nslab, 2, Lc))
        n = (2 * net.lc_ctx + 1) * Lc * Lc
        region('lc_ctx', lib.wn_lc_context_wgrad_slabs(B * ws.lc_fw, n),
               _align4(n), n, own='lc_ctx_slabs')


def parse_cli(scales, hop, context):
    """(scales or None, hop, P or None) of --lc_upsample_scales, --lc_hop
    (None: absent) and --lc_context; ValueError where they do not fit."""
    if scales is None:
        if context is not None:
            raise ValueError('--lc_context needs --lc_upsample_scales (it '
                             'convolves frames)')
        return None, hop, None
    try:
        sc = tuple(int(x) for x in scales.split(','))
    except ValueError:
        raise ValueError('--lc_upsample_scales must be comma-separated ints, '
                         'got %r' % scales)
    prod = int(np.prod(sc))
    if hop is not None and hop != prod:
        raise ValueError('--lc_hop %d disagrees with --lc_upsample_scales %s '
                         '(hop = their product, %d)' % (hop, scales, prod))
    from .model import WaveNetModel
    if context is not None and \
            not 0 <= context <= WaveNetModel.LC_CONTEXT_MAX:
        raise ValueError('--lc_context must be from 0 to %d, got %d'
                         % (WaveNetModel.LC_CONTEXT_MAX, context))
    return sc, prod, context
