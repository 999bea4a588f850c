"""Host-side mirror of the reference's wavenet/ops.py on top of the HIP C ABI.

Same names, argument meaning and error behaviour as
/root/reference/wavenet/ops.py: `optimizer_factory` (:6-24), `time_to_batch`
(:27-34), `batch_to_time` (:37-43), `causal_conv` (:46-62), `mu_law_encode`
(:65-73), `mu_law_decode` (:76-85).  Inputs may be numpy arrays or torch
tensors (the reference's tests pass numpy arrays, test_causal_conv.py:13-17);
results are torch tensors on the GPU.  Every function launches hand-written
HIP kernels; nothing here computes on the CPU.
"""
import math

import numpy as np
import torch

from . import _lib

_TABLES = {}


def _dev():
    _lib.require_gpu()
    return torch.device('cuda', torch.cuda.current_device())


def _as_dev(x, dtype):
    if isinstance(x, torch.Tensor):
        return x.to(device=_dev(), dtype=dtype).contiguous()
    return torch.as_tensor(np.asarray(x), dtype=dtype).to(_dev()).contiguous()


def mu_law_tables(quantization_channels):
    """(thresholds[Q-1], decode_table[Q]) device tensors, cached per (Q, dev).
    Built once on the host by the library from the float32 chain of
    ops.py:65-85 (constant tables, like FFT twiddles -- not a compute path)."""
    dev = _dev()
    key = (int(quantization_channels), dev.index)
    if key not in _TABLES:
        q = int(quantization_channels)
        if q < 2:
            raise ValueError('quantization_channels must be >= 2, got %d' % q)
        thr = np.empty(q - 1, np.float32)
        lut = np.empty(q, np.float32)
        _lib.call('wn_mu_law_thresholds_host', q, thr.ctypes.data)
        _lib.call('wn_mu_law_decode_table_host', q, lut.ctypes.data)
        _TABLES[key] = (torch.from_numpy(thr).to(dev),
                        torch.from_numpy(lut).to(dev))
    return _TABLES[key]


def mu_law_encode(audio, quantization_channels):
    '''Quantizes waveform amplitudes (ops.py:65-73).  int32, same shape.'''
    a = _as_dev(audio, torch.float32)
    out = torch.empty(a.shape, dtype=torch.int32, device=a.device)
    if a.numel() == 0:
        return out
    thr, _ = mu_law_tables(quantization_channels)
    _lib.call('wn_mu_law_encode', _lib.ptr(a), _lib.ptr(out), a.numel(),
              _lib.ptr(thr), int(quantization_channels), _lib.stream())
    return out


def mu_law_decode(output, quantization_channels):
    '''Recovers waveform from quantized values (ops.py:76-85).  float32.'''
    c = _as_dev(output, torch.int32)
    out = torch.empty(c.shape, dtype=torch.float32, device=c.device)
    if c.numel() == 0:
        return out
    _, lut = mu_law_tables(quantization_channels)
    _lib.call('wn_mu_law_decode', _lib.ptr(c), _lib.ptr(out), c.numel(),
              _lib.ptr(lut), int(quantization_channels), _lib.stream())
    return out


def time_to_batch(value, dilation, name=None):
    """ops.py:27-34: [B,T,C] -> [B*dilation, ceil(T/dilation), C]."""
    v = _as_dev(value, torch.float32)
    b, t, c = v.shape
    u = (t + dilation - 1) // dilation
    out = torch.empty((b * dilation, u, c), dtype=torch.float32,
                      device=v.device)
    _lib.call('wn_time_to_batch', _lib.ptr(v), _lib.ptr(out), b, t, c,
              int(dilation), _lib.stream())
    return out


def batch_to_time(value, dilation, name=None):
    """ops.py:37-43: [B*dilation, U, C] -> [B, U*dilation, C]."""
    v = _as_dev(value, torch.float32)
    bd, u, c = v.shape
    if bd % dilation:
        raise ValueError('batch %d not divisible by dilation %d'
                         % (bd, dilation))
    b = bd // dilation
    out = torch.empty((b, u * dilation, c), dtype=torch.float32,
                      device=v.device)
    _lib.call('wn_batch_to_time', _lib.ptr(v), _lib.ptr(out), b, u, c,
              int(dilation), _lib.stream())
    return out


def causal_conv(value, filter_, dilation, name='causal_conv'):
    """ops.py:46-62: value [B,T,Cin], filter_ [K,Cin,Cout] -> [B,T,Cout].
    Any K (incl. TF's 'SAME' centring delay for K > 2), any channel counts."""
    v = _as_dev(value, torch.float32)
    w = _as_dev(filter_, torch.float32)
    if v.dim() != 3 or w.dim() != 3 or v.shape[2] != w.shape[1]:
        raise ValueError('causal_conv: value %s / filter %s mismatch'
                         % (tuple(v.shape), tuple(w.shape)))
    b, t, cin = v.shape
    k, _, cout = w.shape
    out = torch.empty((b, t, cout), dtype=torch.float32, device=v.device)
    _lib.call('wn_causal_conv', _lib.ptr(v), _lib.ptr(w), _lib.ptr(out), b, t,
              cin, cout, k, int(dilation), _lib.stream())
    return out


# ---------------------------------------------------------------------------
# optimizers (ops.py:6-24) with TensorFlow-0.10 update rules
# ---------------------------------------------------------------------------


def _check_clip_ema(clip_norm, ema_decay):
    """Validate the keyword-only arguments of the optimizers (no library or
    device is touched): clip_norm None or a positive finite number, ema_decay
    None or a number in [0, 1).  Returns them as floats (or None)."""
    if clip_norm is not None:
        if isinstance(clip_norm, bool) or not isinstance(
                clip_norm, (int, float, np.integer, np.floating)):
            raise ValueError('clip_norm must be a positive finite number, '
                             'got %r' % (clip_norm,))
        clip_norm = float(clip_norm)
        if not (clip_norm > 0.0 and math.isfinite(clip_norm)):
            raise ValueError('clip_norm must be a positive finite number, '
                             'got %r' % (clip_norm,))
        if clip_norm > float(np.finfo(np.float32).max):
            raise ValueError('clip_norm %r does not fit a float32'
                             % (clip_norm,))
    if ema_decay is not None:
        if isinstance(ema_decay, bool) or not isinstance(
                ema_decay, (int, float, np.integer, np.floating)):
            raise ValueError('ema_decay must lie in [0, 1), got %r'
                             % (ema_decay,))
        ema_decay = float(ema_decay)
        if not (0.0 <= ema_decay < 1.0) or float(np.float32(ema_decay)) >= 1.0:
            raise ValueError('ema_decay must lie in [0, 1), got %r'
                             % (ema_decay,))
    return clip_norm, ema_decay


class _Optimizer(object):
    """Fused flat-buffer optimizer.  `minimize(loss)` mirrors
    tf.train.Optimizer.minimize: `loss` is what WaveNetModel.loss returned
    (its gradients already sit in the model's flat gradient bucket); under
    torch.distributed the bucket is all-reduced (RCCL) and averaged first.

    clip_norm (keyword only): tf.clip_by_global_norm of the averaged global
    gradient (L2 term included: `loss` has added it to the bucket) --
    `wn_grad_norm_partials` after the all-reduce, then the `_clip` update, in
    which every workgroup derives the same factor from the same partials; no
    host wait.  `last_grad_norm` is then a device scalar holding the norm
    before clipping (None without clip_norm).
    ema_decay (keyword only): shadow weights s -= (1 - decay) * (s - p) in the
    same pass, initialised to the parameters before the first update
    (tf.train.ExponentialMovingAverage without num_updates).
    With both None, minimize makes exactly the calls it made before they
    existed."""

    def __init__(self, clip_norm=None, ema_decay=None):
        self.clip_norm, self.ema_decay = _check_clip_ema(clip_norm, ema_decay)
        self._slots = None
        self._shadow = None
        self._gn_parts = None
        self.last_grad_norm = None
        self._step = 0

    def _make_slots(self, model):
        raise NotImplementedError

    _entry = None    # stem of the entry points: wn_<stem>, wn_<stem>_clip

    def _rule_args(self):
        """The entry point's arguments between n and grad_scale."""
        raise NotImplementedError

    def _apply(self, model, grad_scale, clip_tail=None):
        """One update: wn_<stem>, or wn_<stem>_clip with `clip_tail` =
        (partials, nparts, clip_norm, ema, ema_decay, norm_out) in front of
        the stream."""
        name = 'wn_' + self._entry
        tail = (_lib.stream(),)
        if clip_tail is not None:
            name, tail = name + '_clip', tuple(clip_tail) + tail
        _lib.call(name, _lib.ptr(model.params), _lib.ptr(model.grads),
                  *[_lib.ptr(s) for s in self._slots],
                  model.params.numel(), *self._rule_args(),
                  grad_scale, 0.0, None, *tail)

    def init_state(self, model):
        """Create the slots (and, with ema_decay, the shadow as a copy of the
        parameters) for `model` unless they exist."""
        if self._slots is None:
            self._make_slots(model)
        if self.ema_decay is not None and self._shadow is None:
            self._shadow = model.params.detach().clone()

    def minimize(self, loss, var_list=None):
        model = getattr(loss, '_wn_model', None)
        if model is None:
            raise ValueError('minimize() needs the tensor returned by '
                             'WaveNetModel.loss()')
        if not getattr(loss, '_wn_has_grads', False):
            raise ValueError('loss was computed with backward=False')
        from . import parallel
        scale = parallel.allreduce_gradients(model)
        self.init_state(model)
        self._step += 1
        if self.clip_norm is None and self.ema_decay is None:
            self._apply(model, scale)
            return loss
        parts, nparts = None, 0
        if self.clip_norm is not None:
            if self._gn_parts is None:
                nparts = _lib.load().wn_grad_norm_partials_count()
                self._gn_parts = torch.zeros(nparts, dtype=torch.float64,
                                             device=model.params.device)
                self.last_grad_norm = torch.zeros(
                    (), dtype=torch.float32, device=model.params.device)
            parts, nparts = self._gn_parts, self._gn_parts.numel()
            _lib.call('wn_grad_norm_partials', _lib.ptr(model.grads),
                      model.grads.numel(), _lib.ptr(parts), _lib.stream())
        self._apply(model, scale, (
            _lib.ptr(parts), nparts, self.clip_norm or 0.0,
            _lib.ptr(self._shadow), self.ema_decay or 0.0,
            _lib.ptr(self.last_grad_norm)))
        return loss

    # ---- checkpointing ---------------------------------------------------
    def state_dict(self):
        """{'kind', 'step', 'slots', 'shadow'}: the update count (Adam's bias
        correction), the slot buffers and the EMA shadow (None without
        ema_decay) as flat host tensors laid out like model.params."""
        return {'kind': type(self).__name__, 'step': int(self._step),
                'slots': None if self._slots is None else
                [s.detach().cpu().clone() for s in self._slots],
                'shadow': None if self._shadow is None else
                self._shadow.detach().cpu().clone()}

    def load_state_dict(self, sd, model):
        """Restore `state_dict()` for `model` (whose flat parameter layout the
        buffers share).  A state without shadow loaded into an optimizer with
        ema_decay starts the shadow from the model's current parameters."""
        if sd.get('kind') != type(self).__name__:
            raise ValueError('optimizer state of a %s cannot be loaded into a '
                             '%s' % (sd.get('kind'), type(self).__name__))
        n, dev = model.params.numel(), model.params.device
        def flat(t, what):
            t = torch.as_tensor(t, dtype=torch.float32).reshape(-1)
            if t.numel() != n:
                raise ValueError('optimizer %s holds %d floats, the model %d'
                                 % (what, t.numel(), n))
            return t.to(dev).clone()
        self._slots = None
        if sd.get('slots') is not None:
            self._make_slots(model)
            if len(sd['slots']) != len(self._slots):
                raise ValueError('optimizer state holds %d slots, a %s has %d'
                                 % (len(sd['slots']), type(self).__name__,
                                    len(self._slots)))
            self._slots = [flat(s, 'slot') for s in sd['slots']]
        self._shadow = None
        if self.ema_decay is not None and sd.get('shadow') is not None:
            self._shadow = flat(sd['shadow'], 'shadow')
        self._step = int(sd['step'])

    def ema_flat(self, model):
        """The shadow weights as the flat device tensor, laid out like
        model.params (evaluate.parameters_swapped takes it)."""
        if self.ema_decay is None:
            raise ValueError('ema_flat() needs an optimizer built with '
                             'ema_decay')
        self.init_state(model)
        return self._shadow

    def ema_state_dict(self, model):
        """The shadow weights under the keys of model.state_dict() (loadable
        with model.load_state_dict)."""
        if self.ema_decay is None:
            raise ValueError('ema_state_dict() needs an optimizer built with '
                             'ema_decay')
        self.init_state(model)
        return {n: v.detach().cpu().clone() for n, v in
                model.named_variables(model._views(self._shadow))}


class AdamOptimizer(_Optimizer):
    # tf.train.AdamOptimizer(learning_rate, epsilon=1e-4); `momentum` ignored
    _entry = 'adam'

    def __init__(self, learning_rate, epsilon=1e-4, beta1=0.9, beta2=0.999,
                 *, clip_norm=None, ema_decay=None):
        super(AdamOptimizer, self).__init__(clip_norm, ema_decay)
        self.lr, self.eps, self.b1, self.b2 = learning_rate, epsilon, beta1, beta2

    def _make_slots(self, model):
        self._slots = [torch.zeros_like(model.params),
                       torch.zeros_like(model.params)]

    def _rule_args(self):
        t = self._step
        lr_t = self.lr * math.sqrt(1.0 - self.b2 ** t) / (1.0 - self.b1 ** t)
        return lr_t, self.b1, self.b2, self.eps


class MomentumOptimizer(_Optimizer):
    _entry = 'momentum'

    def __init__(self, learning_rate, momentum, *, clip_norm=None,
                 ema_decay=None):
        super(MomentumOptimizer, self).__init__(clip_norm, ema_decay)
        self.lr, self.mom = learning_rate, momentum

    def _make_slots(self, model):
        self._slots = [torch.zeros_like(model.params)]

    def _rule_args(self):
        return self.lr, self.mom


class RMSPropOptimizer(_Optimizer):
    # tf.train.RMSPropOptimizer(lr, decay=0.9, momentum, epsilon=1e-5);
    # the `rms` slot starts at ONE (TensorFlow), `momentum` slot at zero.
    _entry = 'rmsprop'

    def __init__(self, learning_rate, momentum, epsilon=1e-5, decay=0.9, *,
                 clip_norm=None, ema_decay=None):
        super(RMSPropOptimizer, self).__init__(clip_norm, ema_decay)
        self.lr, self.mom, self.eps, self.decay = (learning_rate, momentum,
                                                   epsilon, decay)

    def _make_slots(self, model):
        self._slots = [torch.ones_like(model.params),
                       torch.zeros_like(model.params)]

    def _rule_args(self):
        return self.lr, self.decay, self.mom, self.eps


def create_adam_optimizer(learning_rate, momentum, *, clip_norm=None,
                          ema_decay=None):
    return AdamOptimizer(learning_rate=learning_rate, epsilon=1e-4,
                         clip_norm=clip_norm, ema_decay=ema_decay)


def create_sgd_optimizer(learning_rate, momentum, *, clip_norm=None,
                         ema_decay=None):
    return MomentumOptimizer(learning_rate=learning_rate, momentum=momentum,
                             clip_norm=clip_norm, ema_decay=ema_decay)


def create_rmsprop_optimizer(learning_rate, momentum, *, clip_norm=None,
                             ema_decay=None):
    return RMSPropOptimizer(learning_rate=learning_rate, momentum=momentum,
                            epsilon=1e-5, clip_norm=clip_norm,
                            ema_decay=ema_decay)


optimizer_factory = {'adam': create_adam_optimizer,
                     'sgd': create_sgd_optimizer,
                     'rmsprop': create_rmsprop_optimizer}
