"""Input noise on the device: perturbed mu-law codes for the network to read
while the loss keeps the clean codes as targets (csrc/wn_misc.hip).

Under teacher forcing row t of a training pass always sees the true codes
q[..t]; a generating model sees its own draws.  `InputNoise(prob, width)`
moves a fraction `prob` of the INPUT codes by a triangular step in the mu-law
domain, so that the model learns to predict the true next sample from a
slightly wrong past.  The rule, integer arithmetic only -- device and
`reference` agree bit for bit:

    thresh = int(prob * 2**24)                  (prob = 1: 2**24, always)
    c      = (k[b] << 24) | t                   k[b]: clip b's key, < 2**40
    bits   = draw_bits(seed ^ 0x6e6f697365, c)  (csrc/wn_common.h)
    hit    = (bits & 0xFFFFFF) < thresh
    d      = ((bits >> 24) & 0xFFFFF) % (w + 1) - ((bits >> 44) & 0xFFFFF) % (w + 1)
    q_in[b][t] = clamp(q[b][t] + d, 0, Q - 1)   where hit, t < n[b] and
                                                0 <= q[b][t] < Q
                 q[b][t]                        otherwise

with w = width, n[b] = lengths[b] (T without lengths), t < 2**24.  d is
triangular on [-w, w] (variance w (w + 2) / 6).  The padding, out-of-range
codes and prob = 0 pass through; history rows are inputs like any other and
are perturbed.  What a position draws is a pure function of (seed, key, t):
`step_keys` gives every clip of every step and rank its own key, so a resumed
run draws what the uninterrupted run drew.

train.py --input_noise P,W stores `entry()` in every checkpoint under
'input_noise'; evaluate.py --input_noise P,W scores a set a second time with
perturbed inputs.  Models with scalar_input read float audio, not codes: they
take no input noise.
"""
import math

import numpy as np

from . import _lib
from .corpus import draw_bits
from .features import check_lengths

SEED_TAG = 0x6e6f697365
KEY_LIMIT = 1 << 40             # keys lie below it
T_LIMIT = 1 << 24               # positions lie below it
WIDTH_MAX = 4095
_RING = 4                       # pinned staging rows per (device, batch size)


def _is_int(v):
    return isinstance(v, (int, np.integer)) and \
        not isinstance(v, (bool, np.bool_))


def step_keys(step, B, rank=0, world=1):
    """The keys of step `step`'s B clips on rank `rank` of `world`:
    (step * B + arange(B)) * world + rank, int64 [B].  Distinct over
    (step, b, rank); ValueError where one would reach 2**40."""
    for name, v, lo in (('step', step, 0), ('B', B, 1), ('rank', rank, 0),
                        ('world', world, 1)):
        if not _is_int(v) or v < lo:
            raise ValueError('step_keys: %s must be an int >= %d, got %r'
                             % (name, lo, v))
    if rank >= world:
        raise ValueError('step_keys: rank %d of world %d' % (rank, world))
    last = (int(step) * int(B) + int(B) - 1) * int(world) + int(rank)
    if last >= KEY_LIMIT:
        raise ValueError('step_keys: key %d of step %d reaches 2**40'
                         % (last, step))
    return (int(step) * int(B) + np.arange(int(B), dtype=np.int64)) \
        * int(world) + int(rank)


def _check_keys(keys, B, what):
    """Host keys as int64 numpy [B] (checked), a device tensor as it is."""
    if hasattr(keys, 'detach') and keys.device.type != 'cpu':
        if str(keys.dtype) != 'torch.int64' or tuple(keys.shape) != (B,):
            raise ValueError('%s: device keys must be int64 [%d], got %s %s'
                             % (what, B, keys.dtype, tuple(keys.shape)))
        return keys
    if hasattr(keys, 'detach'):
        keys = keys.detach().numpy()
    k = np.asarray(keys)
    if k.dtype == object or k.dtype == np.bool_ or \
            not np.issubdtype(k.dtype, np.integer) or k.shape != (B,):
        raise ValueError('%s: keys must be %d integers, got %s %s'
                         % (what, B, k.dtype, list(k.shape)))
    if (k < 0).any() or (k >= KEY_LIMIT).any():
        raise ValueError('%s: keys must lie in [0, 2**40), got %s'
                         % (what, k.tolist()))
    return k.astype(np.int64)


def _shape2(x, what):
    shape = tuple(int(v) for v in x.shape)
    if len(shape) != 2 or min(shape) < 1 or shape[1] > T_LIMIT:
        raise ValueError('%s needs a [B, T] array with B >= 1 and '
                         '1 <= T <= 2**24, got shape %s' % (what, shape))
    return shape


class InputNoise(object):
    """The noise of one (prob, width, seed) (module docstring): 0 <= prob <=
    1 a finite number, width an int in [1, 4095], seed an int in [0, 2**64).
    Every argument is checked before the library or a device is touched."""

    def __init__(self, prob, width, seed=0):
        if isinstance(prob, (bool, np.bool_)) or \
                not isinstance(prob, (int, float, np.integer, np.floating)) \
                or not math.isfinite(float(prob)) or \
                not 0.0 <= float(prob) <= 1.0:
            raise ValueError('prob must be a finite number in [0, 1], got %r'
                             % (prob,))
        if not _is_int(width) or not 1 <= width <= WIDTH_MAX:
            raise ValueError('width must be an int in [1, %d], got %r'
                             % (WIDTH_MAX, width))
        if not _is_int(seed) or not 0 <= seed < 1 << 64:
            raise ValueError('seed must be an int in [0, 2**64), got %r'
                             % (seed,))
        self.prob, self.width, self.seed = float(prob), int(width), int(seed)
        self.thresh = int(self.prob * float(1 << 24))   # what the kernels get
        self._pins, self._turn = {}, 0      # pinned staging rows (_stage)

    def __repr__(self):
        return 'InputNoise(%r, %r, seed=%r)' % (self.prob, self.width,
                                                self.seed)

    def __eq__(self, other):
        return isinstance(other, InputNoise) and \
            (other.prob, other.width, other.seed) == \
            (self.prob, self.width, self.seed)

    def __ne__(self, other):
        return not self == other

    __hash__ = None

    # ------------------------------------------------------- checkpoint form
    def entry(self):
        """What checkpoints store under 'input_noise'."""
        return {'prob': self.prob, 'width': self.width, 'seed': self.seed}

    @classmethod
    def from_entry(cls, d):
        """The InputNoise of a checkpoint's entry; None for None."""
        if d is None:
            return None
        if not isinstance(d, dict) or 'prob' not in d or 'width' not in d:
            raise ValueError("an input_noise entry needs 'prob' and 'width', "
                             'got %r' % (d,))
        return cls(d['prob'], d['width'], d.get('seed', 0))

    # ------------------------------------------------------- the rule, numpy
    def reference(self, q, keys, lengths, Q):
        """q_in of the rule in numpy: q int [B, T], keys B ints, lengths B
        ints in [1, T] or None; int32 [B, T]."""
        q = np.asarray(q)
        B, T = _shape2(q, 'reference')
        k = _check_keys(np.asarray(keys), B, 'reference')
        n = check_lengths(lengths, B, T, 'reference')
        n = np.full(B, T, np.int64) if n is None else n.astype(np.int64)
        q = q.astype(np.int64)
        t = np.arange(T, dtype=np.uint64)
        c = (k.astype(np.uint64)[:, None] << np.uint64(24)) | t[None, :]
        bits = draw_bits(self.seed ^ SEED_TAG, c)
        w1 = np.uint64(self.width + 1)
        m20 = np.uint64(0xFFFFF)
        hit = (bits & np.uint64(0xFFFFFF)).astype(np.int64) < self.thresh
        d = (((bits >> np.uint64(24)) & m20) % w1).astype(np.int64) - \
            (((bits >> np.uint64(44)) & m20) % w1).astype(np.int64)
        move = hit & (t.astype(np.int64)[None, :] < n[:, None]) & \
            (q >= 0) & (q < Q)
        return np.where(move, np.clip(q + d, 0, Q - 1), q).astype(np.int32)

    # ------------------------------------------------------------ the device
    def _stage(self, like, keys, lengths, B, T, what):
        """keys int64 [B] and lengths int32 [B] (or None) on like's device.
        What comes from the host goes up in ONE copy from a pinned row of a
        small ring, asynchronously: the call does not wait for the device
        (a pageable copy would, for everything queued before it)."""
        import torch
        n = check_lengths(lengths, B, T, what)
        on_dev = isinstance(keys, torch.Tensor)
        if on_dev:
            keys = keys.to(like.device).contiguous()
            if n is None:
                return keys, None
        # int64 words: the keys, then the lengths as int32 pairs
        words = B + (B + 1) // 2
        ring = self._pins.setdefault((like.device, words), [])
        if len(ring) < _RING:
            ring.append((torch.empty(words, dtype=torch.int64).pin_memory(),
                         torch.cuda.Event()))
            host, done = ring[-1]
        else:
            self._turn = (self._turn + 1) % _RING
            host, done = ring[self._turn]
            done.synchronize()      # (this row's last upload, long past)
        if not on_dev:
            host[:B].copy_(torch.from_numpy(keys))
        if n is not None:
            host[B:].view(torch.int32)[:B].copy_(torch.from_numpy(n))
        dev = torch.empty(words, dtype=torch.int64, device=like.device)
        dev.copy_(host, non_blocking=True)
        done.record()
        return (keys if on_dev else dev[:B],
                None if n is None else dev[B:].view(torch.int32)[:B])

    def codes(self, q, keys, lengths=None, *, Q=256, out=None):
        """q_in for codes q (int [B, T], an array or a device tensor): device
        int32 [B, T], without waiting for the device.  keys: B ints in
        [0, 2**40) (a host array, staged per call) or a device int64 [B]
        tensor; lengths: B ints in [1, T] or None; Q: the model's
        quantization_channels (codes outside [0, Q) pass through, the others
        are clamped to it; default: the 8-bit mu-law path's 256); out: a
        contiguous device int32 [B, T] tensor to write into (it may be q
        itself)."""
        _check_Q(Q, 'codes')
        if not hasattr(q, 'detach'):
            q = np.asarray(q)
            if q.dtype == object or not np.issubdtype(q.dtype, np.integer):
                raise ValueError('codes: q must hold integers, got %s'
                                 % q.dtype)
        elif q.is_floating_point():
            raise ValueError('codes: q must hold integers, got %s' % q.dtype)
        B, T = _shape2(q, 'codes')
        keys = _check_keys(keys, B, 'codes')
        check_lengths(lengths, B, T, 'codes')
        _check_out(out, B, T, 'codes')
        import torch
        _lib.load()
        _lib.require_gpu()
        if isinstance(q, torch.Tensor) and q.device.type == 'cuda':
            device = q.device
        else:
            device = out.device if out is not None else \
                torch.device('cuda', torch.cuda.current_device())
            if not isinstance(q, torch.Tensor):
                q = torch.from_numpy(np.ascontiguousarray(q))
        src = q.to(device=device, dtype=torch.int32).contiguous()
        dst = out if out is not None else torch.empty_like(src)
        kd, nd = self._stage(src, keys, lengths, B, T, 'codes')
        with torch.cuda.device(device):
            _lib.call('wn_code_noise', _lib.ptr(src), _lib.ptr(dst),
                      _lib.ptr(kd), _lib.ptr(nd), B, T, int(Q), self.seed,
                      self.thresh, self.width, _lib.stream())
        return dst

    def encode(self, audio, Q, keys, lengths=None, out=None):
        """(q, q_in) for float audio [B, T] (an array or a device tensor)
        through the fused kernel: the mu-law codes of ops.mu_law_encode and
        their perturbed copy, device int32 [B, T] each, without waiting for
        the device.  keys, lengths: as for `codes`; out: a pair of contiguous
        device int32 [B, T] tensors (q, q_in) to write into."""
        if hasattr(audio, 'detach'):
            ok = audio.is_floating_point()
        else:
            audio = np.asarray(audio)
            ok = audio.dtype != object and \
                np.issubdtype(audio.dtype, np.floating)
        if not ok:
            raise ValueError('encode: audio must hold floats, got %s'
                             % audio.dtype)
        B, T = _shape2(audio, 'encode')
        _check_Q(Q, 'encode')
        keys = _check_keys(keys, B, 'encode')
        check_lengths(lengths, B, T, 'encode')
        if out is not None:
            if not isinstance(out, (tuple, list)) or len(out) != 2:
                raise ValueError('encode: out must be a pair (q, q_in)')
            for o in out:
                _check_out(o, B, T, 'encode')
            if out[0].data_ptr() == out[1].data_ptr():
                raise ValueError('encode: out needs two buffers')
        import torch
        from .ops import mu_law_tables
        _lib.load()
        _lib.require_gpu()
        if isinstance(audio, torch.Tensor) and audio.device.type == 'cuda':
            device = audio.device
        else:
            device = out[0].device if out is not None else \
                torch.device('cuda', torch.cuda.current_device())
            if not isinstance(audio, torch.Tensor):
                audio = torch.from_numpy(np.ascontiguousarray(audio))
        a = audio.to(device=device, dtype=torch.float32).contiguous()
        if out is not None:
            q, q_in = out
        else:
            q = torch.empty((B, T), dtype=torch.int32, device=device)
            q_in = torch.empty_like(q)
        kd, nd = self._stage(a, keys, lengths, B, T, 'encode')
        with torch.cuda.device(device):
            thr, _ = mu_law_tables(Q)
            _lib.call('wn_mu_law_encode_noisy', _lib.ptr(a), _lib.ptr(q),
                      _lib.ptr(q_in), _lib.ptr(kd), _lib.ptr(nd), B, T,
                      _lib.ptr(thr), int(Q), self.seed, self.thresh,
                      self.width, _lib.stream())
        return q, q_in


def _check_Q(Q, what):
    if not _is_int(Q) or Q < 2:
        raise ValueError('%s: Q must be an int >= 2, got %r' % (what, Q))


def _check_out(out, B, T, what):
    if out is None:
        return
    if not hasattr(out, 'detach') or str(out.dtype) != 'torch.int32' or \
            tuple(out.shape) != (B, T) or out.device.type != 'cuda' or \
            not out.is_contiguous():
        raise ValueError('%s: out must be a contiguous int32 device tensor '
                         'of shape %s' % (what, (B, T)))


# ------------------------------------------------------------ command line
def parse_flag(value):
    """(prob, width) of an --input_noise value 'P,W'; ValueError otherwise."""
    parts = str(value).split(',')
    if len(parts) != 2:
        raise ValueError('expected P,W (a probability and a width, e.g. '
                         '0.5,2), got %r' % (value,))
    try:
        prob, width = float(parts[0]), int(parts[1])
    except ValueError:
        raise ValueError('expected P,W (a probability and an integer width, '
                         'e.g. 0.5,2), got %r' % (value,))
    return prob, width


def add_cli_flags(p, train=False):
    p.add_argument(
        '--input_noise', type=str, default=None, metavar='P,W',
        help=('Perturb the network\'s INPUT codes during training: each '
              'position with probability P by a triangular step of at most W '
              'mu-law codes; the targets stay clean (wavenet/'
              'input_noise.py).  Stored in every checkpoint '
              '(\'input_noise\').  Validation stays clean.  Default: off.')
        if train else
        ('Score the set a second time with perturbed input codes '
         '(probability P, width W; clean targets) and add "noisy_input" to '
         'the JSON line: the gap to the clean numbers says how much the '
         'model depends on an exact past.  Default: off.'))
    p.add_argument('--input_noise_seed', type=int, default=None, metavar='S',
                   help='seed of --input_noise, in [0, 2**64) (default 0)')


def from_cli(p, args):
    """The InputNoise of parsed --input_noise / --input_noise_seed, or None;
    a malformed value is an argparse error of `p` that names the flag."""
    if args.input_noise is None:
        if args.input_noise_seed is not None:
            p.error('--input_noise_seed needs --input_noise')
        return None
    seed = args.input_noise_seed or 0
    if not 0 <= seed < 1 << 64:
        p.error('--input_noise_seed: must lie in [0, 2**64), got %d' % seed)
    try:
        prob, width = parse_flag(args.input_noise)
        return InputNoise(prob, width, seed)
    except ValueError as e:
        p.error('--input_noise: %s' % e)
