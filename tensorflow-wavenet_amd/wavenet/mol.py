"""Mixture-of-logistics output head over 65536 levels, host side
(csrc/wn_mol.hip, include/wavenet_mol.h): the head's layout and limits, the
rule restated in numpy (levels_reference, loss_reference, sample_reference),
the launches WaveNetModel and scoring.py make in the place of wn_xent*, and
the checkpoint entry the command-line tools keep.

A model built with output_mixture=K reads float audio snapped to the 16-bit
grid (the centres c(j)) and ends in 3 Kp columns [pi | mu | beta_raw], Kp = K
rounded up to a multiple of 4; row t is scored on the level j[t + 1].
Functions that launch take the model first."""
import numpy as np
import torch

from . import _lib

LEVELS = 65536
TOP = LEVELS - 1
MAX_COMPONENTS = 32
LOG_SCALE_MIN_RANGE = (-32.0, -1.0)
# what stays refused for these models, named in every such error
FOLLOW_UP = ('a mixture model generates fast through generate_mixture / '
             'generate_mixture_batch (generate.py --fast_mixture true); the '
             'single-stream persistent kernels, bulk synthesis and '
             'evaluate.py --synthesis for mixture models, and scalar-input '
             'softmax models, are the follow-up; generate naively '
             '(generate.py --fast_generation false)')
_M64 = (1 << 64) - 1


def padded(K):
    """Kp: K rounded up to a multiple of 4."""
    return (int(K) + 3) // 4 * 4


def check_config(K, log_scale_min, scalar_input):
    """The constructor's output_mixture / mixture_log_scale_min, checked on
    the host.  Returns (K, float log_scale_min)."""
    if isinstance(K, (bool, np.bool_)) or \
            not isinstance(K, (int, np.integer)) or \
            not 1 <= int(K) <= MAX_COMPONENTS:
        raise ValueError('output_mixture must be an int from 1 to %d, got %r'
                         % (MAX_COMPONENTS, K))
    if not scalar_input:
        raise ValueError('output_mixture needs scalar_input=True: the '
                         'network reads the 16-bit centres as float audio')
    lo, hi = LOG_SCALE_MIN_RANGE
    x = log_scale_min
    if isinstance(x, (bool, np.bool_)) or \
            not isinstance(x, (int, float, np.integer, np.floating)) or \
            not lo <= float(x) <= hi:
        raise ValueError('mixture_log_scale_min must be a number from %g to '
                         '%g, got %r' % (lo, hi, x))
    return int(K), float(x)


# ------------------------------------------------------------ the rule, numpy
def centres(levels):
    """c(j) = float32(2 j - 65535) / 65535: one rounded division."""
    j = np.asarray(levels).astype(np.int64)
    return (2 * j - TOP).astype(np.float32) / np.float32(TOP)


def levels_reference(audio, lengths=None):
    """wn_mol_quantize in numpy float32, bit for bit: (levels int32, centres
    float32) of audio [B, T] (or [T]); samples at or behind lengths[b] give
    level 0 and centre 0."""
    y = np.asarray(audio, np.float32)
    y = np.fmin(np.fmax(y, np.float32(-1)), np.float32(1))
    t = y + np.float32(1)
    t = t * np.float32(32767.5)
    j = np.rint(t).astype(np.int32)
    c = centres(j)
    if lengths is not None:
        T = y.shape[-1]
        n = np.clip(np.asarray(lengths, np.int64), 0, T)
        keep = np.arange(T)[None, :] < n[:, None]
        j = np.where(keep, j, 0).astype(np.int32)
        c = np.where(keep, c, np.float32(0)).astype(np.float32)
    return j, c


def _fold(x, reduce, K, empty):
    """Sum or maximum over the components (last axis, K of them) in the
    kernel's order: component k = 4 i + s belongs to lane s, a lane folds its
    i ascending, the lanes combine as (s0 + s1) + (s2 + s3)."""
    pad = np.full(x.shape[:-1] + (32 - K,), empty, x.dtype)
    v = np.concatenate([x, pad], -1).reshape(x.shape[:-1] + (8, 4))
    acc = v[..., 0, :]
    for i in range(1, 8):
        acc = reduce(acc, v[..., i, :])
    return reduce(reduce(acc[..., 0], acc[..., 1]),
                  reduce(acc[..., 2], acc[..., 3]))


def loss_reference(logits, target, K, log_scale_min, inv, dtype=np.float64):
    """The row loss of include/wavenet_mol.h in numpy, operation for
    operation, in `dtype`: float64 is the kernel's arithmetic (its outputs
    are these rounded to float32, up to the library functions' last bits);
    float32 is what the same chain gives in single precision, the yardstick
    the kernel tests hold the device against.  logits [N, >= 3 Kp]; target
    int [N], a level or -1 for a row without one; inv: the gradient's
    scale.  Returns (nll [N], dlogits [N, 3 Kp]), zeros in rows without a
    target."""
    f = dtype
    K, Kp = int(K), padded(K)
    lg = np.asarray(logits)[:, :3 * Kp].astype(f)
    j = np.asarray(target).astype(np.int64)
    has = (j >= 0) & (j <= TOP)
    jj = np.where(has, j, 1)
    lsm, inv = f(log_scale_min), f(inv)
    h, h2 = f(1) / f(TOP), f(2) / f(TOP)
    log2h = np.log(h2)
    c = ((2 * jj - TOP).astype(f) / f(TOP))[:, None]
    pi, mu, braw = lg[:, :K], lg[:, Kp:Kp + K], lg[:, 2 * Kp:2 * Kp + K]
    with np.errstate(over='ignore', divide='ignore', invalid='ignore'):
        beta = np.maximum(braw, lsm)
        is_ = np.exp(-beta)
        d = c - mu
        a, b = (d + h) * is_, (d - h) * is_
        D = h2 * is_
        ea, eb = np.exp(-np.abs(a)), np.exp(-np.abs(b))
        spa = np.maximum(-a, f(0)) + np.log1p(ea)
        spb = np.maximum(b, f(0)) + np.log1p(eb)
        sna = np.where(a <= 0, f(1) / (f(1) + ea), ea / (f(1) + ea))
        sb = np.where(b >= 0, f(1) / (f(1) + eb), eb / (f(1) + eb))
        q = np.where(D > 0, -np.expm1(-D) / np.where(D > 0, D, f(1)), f(1))
        lt = np.where(D >= 1, np.log(-np.expm1(-np.where(D >= 1, D, f(1)))),
                      (log2h - beta) + np.log(q))
        gt = np.where(D > 0, D / np.expm1(np.where(D > 0, D, f(1))), f(1))
        lo, hi = (jj == 0)[:, None], (jj == TOP)[:, None]
        lp = np.where(lo, -spa, np.where(hi, -spb, (-spa - spb) + lt))
        dmu = np.where(lo, -(is_ * sna), np.where(hi, is_ * sb,
                                                  is_ * (sb - sna)))
        dbe = np.where(lo, -(a * sna), np.where(hi, b * sb,
                                                (b * sb - a * sna) - gt))
        dbe = np.where(braw < lsm, f(0), dbe)
        mp = _fold(pi, np.maximum, K, f(-np.inf))[:, None]
        pim = pi - mp
        sp = _fold(np.exp(pim), np.add, K, f(0))[:, None]
        w = (pim - np.log(sp)) + lp
        mw = _fold(w, np.maximum, K, f(-np.inf))[:, None]
        ew = np.exp(w - mw)
        sw = _fold(ew, np.add, K, f(0))[:, None]
        nll = -(mw + np.log(sw))[:, 0]
        r, p = ew / sw, np.exp(pim) / sp
        g = np.zeros((lg.shape[0], 3 * Kp), f)
        g[:, :K] = (p - r) * inv
        g[:, Kp:Kp + K] = -(r * dmu) * inv
        g[:, 2 * Kp:2 * Kp + K] = -(r * dbe) * inv
    nll = np.where(has, nll, f(0)).astype(f)
    g[~has] = 0
    return nll, g


def params_reference(row, K, log_scale_min):
    """wn_mol_params_row in numpy: [3, K] float32."""
    K, Kp = int(K), padded(K)
    row = np.asarray(row, np.float32)
    pi = row[:K].astype(np.float64)
    m, se = pi.max(), 0.0
    for k in range(K):
        se += np.exp(pi[k] - m)
    out = np.empty((3, K), np.float32)
    out[0] = ((pi - m) - np.log(se)).astype(np.float32)
    out[1] = row[Kp:Kp + K]
    out[2] = np.maximum(row[2 * Kp:2 * Kp + K], np.float32(log_scale_min))
    return out


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def draw_uniform(seed, counter):
    """draw_uniform of csrc/wn_common.h on Python ints: 53 bits of
    splitmix64(seed ^ splitmix64(counter)) as a float in [0, 1)."""
    bits = _splitmix64((int(seed) & _M64) ^ _splitmix64(int(counter) & _M64))
    return float(bits >> 11) * 2.0 ** -53


def sample_reference(params, seeds, counters, temperature, uniforms=None,
                     return_x=False):
    """wn_mol_sample in numpy float64: params [R, 3, K] float32 -> (levels
    int32 [R], centres float32 [R]).  A pure function of its arguments: row
    r draws u1, u2 from (seeds[r], counters[r]) alone.  uniforms [R, 2]
    replaces the two draws (the host tests force their bits); return_x: also
    the float64 x before the clamp."""
    p = np.asarray(params, np.float32)
    R, _, K = p.shape
    tau = float(np.float32(temperature))
    lv, xs = np.empty(R, np.int32), np.empty(R, np.float64)
    for r in range(R):
        if uniforms is None:
            u1 = draw_uniform(seeds[r], 2 * int(counters[r]))
            u2 = draw_uniform(seeds[r], 2 * int(counters[r]) + 1)
        else:
            u1, u2 = float(uniforms[r][0]), float(uniforms[r][1])
        pk = np.exp(p[r, 0].astype(np.float64))
        total = 0.0
        for k in range(K):
            total += pk[k]
        t, cum, pick, last = u1 * total, 0.0, -1, 0
        for k in range(K):
            cum += pk[k]
            if pk[k] > 0.0:
                last = k
            if pick < 0 and t < cum:
                pick = k
        if pick < 0:
            pick = last
        x = np.float64(p[r, 1, pick])
        if tau != 0.0:
            sc = np.exp(np.float64(p[r, 2, pick])) * np.float64(tau)
            with np.errstate(divide='ignore'):
                lg = np.log(np.float64(u2)) - np.log(np.float64(1.0) -
                                                     np.float64(u2))
            x = x + sc * lg
        xs[r] = x
        x = np.fmin(np.fmax(x, -1.0), 1.0)
        q = x + 1.0
        q = q * 32767.5
        lv[r] = int(np.rint(q))
    out = (lv, centres(lv))
    return out + (xs,) if return_x else out


# ------------------------------------------------------------------ launches
def quantize(audio, lengths, levels_out, centres_out):
    """wn_mol_quantize: audio device float32 [B, T] (contiguous), lengths
    device int32 [B] or None, into the two device buffers."""
    B, T = audio.shape
    _lib.call('wn_mol_quantize', _lib.ptr(audio), _lib.ptr(lengths),
              _lib.ptr(levels_out), _lib.ptr(centres_out), B, T,
              _lib.stream())


def stage(net, ws, a, mask):
    """The float audio a [B, T] of a loss / score call into workspace ws:
    the centres into ws.audio, which the network reads, and the levels into
    ws.q, where the labels go.  mask: model.check_lengths' or None."""
    lengths = None
    if mask is not None:
        # (the lengths as the loss launch will read them: same buffer)
        lengths = ws.xent_mask[:ws.B]
        lengths.copy_(torch.from_numpy(mask[0]))
    quantize(a.contiguous(), lengths, ws.q, ws.audio)


def loss(net, ws, masked, hist, backward):
    """wn_mol_loss on ws.logits in the place of wn_xent / _masked / _window:
    ws.xent_mask (lengths, then 1 / den) and ws.xent_hist are staged by the
    caller as for those."""
    B = ws.B
    _lib.call('wn_mol_loss', _lib.ptr(ws.logits), net.Q, _lib.ptr(ws.q),
              _lib.ptr(ws.xent_hist) if hist else None,
              _lib.ptr(ws.xent_mask) if masked else None,
              _lib.ptr(ws.xent_mask[B:]) if masked else None,
              _lib.ptr(ws.logits) if backward else None,
              _lib.ptr(ws.loss_parts[2:]), B, ws.T, net.mol_K,
              net.mol_log_scale_min, _lib.stream())


def score(net, ws, lengths, hist, rows, nll, count):
    """wn_mol_score on ws.logits (scoring.score's buffers)."""
    if getattr(ws, 'score_scratch', None) is None:
        ws.score_scratch = torch.empty(
            int(_lib.load().wn_mol_score_scratch_floats(ws.N)),
            dtype=torch.float32, device=net.device)
    _lib.call('wn_mol_score', _lib.ptr(ws.logits), net.Q, _lib.ptr(ws.q),
              _lib.ptr(hist), _lib.ptr(lengths), _lib.ptr(rows),
              _lib.ptr(nll), _lib.ptr(count), _lib.ptr(ws.score_scratch),
              ws.B, ws.T, net.mol_K, net.mol_log_scale_min, _lib.stream())


def params_row(net, logits_row):
    """[3, K] float32 (log_softmax(pi), mu, clamped beta) of one row."""
    out = torch.empty((3, net.mol_K), dtype=torch.float32, device=net.device)
    _lib.call('wn_mol_params_row', _lib.ptr(logits_row), net.mol_K,
              net.mol_log_scale_min, _lib.ptr(out), _lib.stream())
    return out


def sample(params, seeds, counters, temperature):
    """wn_mol_sample: params device float32 [R, 3, K]; seeds, counters: R
    ints.  Returns device (levels int32 [R], centres float32 [R])."""
    R, _, K = params.shape
    dev = params.device

    def u64(v):
        a = np.array([int(x) & _M64 for x in np.atleast_1d(v)], np.uint64)
        return torch.from_numpy(a.view(np.int64)).to(dev)
    s, c = u64(seeds), u64(counters)
    if s.numel() != R or c.numel() != R:
        raise ValueError('sample: %d rows need %d seeds and counters'
                         % (R, R))
    t = float(temperature)
    if not (t >= 0.0 and np.isfinite(t)):
        raise ValueError('sample: temperature must be finite and >= 0, got '
                         '%r' % (temperature,))
    lv = torch.empty(R, dtype=torch.int32, device=dev)
    ce = torch.empty(R, dtype=torch.float32, device=dev)
    _lib.call('wn_mol_sample', _lib.ptr(params.contiguous()), _lib.ptr(s),
              _lib.ptr(c), t, _lib.ptr(lv), _lib.ptr(ce), R, K,
              _lib.stream())
    return lv, ce


# ---------------------------------------------------------- command line
def add_cli_flags(p):
    """train.py's --output_mixture / --mixture_log_scale_min."""
    p.add_argument('--output_mixture', type=int, default=None, metavar='K',
                   help='End the network in a discretised mixture of K '
                        'logistics over 65536 levels (1 to %d) instead of '
                        'the softmax over mu-law codes.  Needs '
                        '"scalar_input": true in --wavenet_params.  Stored '
                        'in every checkpoint; generate.py and evaluate.py '
                        'read it there.  Default: off.' % MAX_COMPONENTS)
    p.add_argument('--mixture_log_scale_min', type=float, default=None,
                   metavar='X',
                   help='--output_mixture: the floor of a component\'s log '
                        'scale, from %g to %g.  Default: -14.'
                   % LOG_SCALE_MIN_RANGE)


def from_cli(p, args):
    """(K, log_scale_min) of the flags, or None without --output_mixture;
    argparse errors where they do not fit the --wavenet_params file."""
    K, lsm = args.output_mixture, args.mixture_log_scale_min
    if K is None:
        if lsm is not None:
            p.error('--mixture_log_scale_min needs --output_mixture')
        return None
    import json
    with open(args.wavenet_params, 'r') as f:
        scalar = bool(json.load(f).get('scalar_input'))
    if not scalar:
        p.error('--output_mixture needs "scalar_input": true in '
                '--wavenet_params (%s): the network reads the 16-bit '
                'centres as float audio' % args.wavenet_params)
    try:
        return check_config(K, -14.0 if lsm is None else lsm, True)
    except ValueError as e:
        p.error('--output_mixture / --mixture_log_scale_min: %s' % e)


def model_keywords(head):
    """The WaveNetModel keywords of from_cli's / check_entry's result."""
    if head is None:
        return {}
    return dict(output_mixture=head[0], mixture_log_scale_min=head[1])


# ------------------------------------------------- the checkpoints' entry
def output_entry(K, log_scale_min):
    """What train.py stores under 'output' in every checkpoint."""
    return {'kind': 'mol', 'components': int(K),
            'log_scale_min': float(log_scale_min), 'levels': LEVELS}


def check_entry(entry):
    """A checkpoint's 'output' entry (or None), checked: (K, log_scale_min)
    or None for a softmax model."""
    if entry is None:
        return None
    if not isinstance(entry, dict) or entry.get('kind') != 'mol' or \
            entry.get('levels') != LEVELS:
        raise ValueError("unknown 'output' entry in the checkpoint: %r"
                         % (entry,))
    K, lsm = check_config(entry.get('components'),
                          entry.get('log_scale_min'), True)
    return K, lsm


def same_entry(stored, K, log_scale_min):
    """Continuing a run: the flags must agree with what the checkpoint was
    trained with (either may be None: a softmax head)."""
    now = None if K is None else output_entry(K, log_scale_min)
    if stored != now:
        raise ValueError('the checkpoint was trained with output %r, this '
                         'run asks for %r' % (stored, now))
