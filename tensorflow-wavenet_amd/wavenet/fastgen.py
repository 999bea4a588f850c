"""Fast generation, host side (_create_generator, predict_proba_incremental,
wavenet/model.py:444-626; the loop of generate.py:195-241): the queues of one
stream (`net._gen`) or of B streams in lock step (`net._bgen`) stay on the
device.  Library entry points are looked up when they run."""
import functools
import warnings

import numpy as np
import torch

from . import _lib
from . import local_condition as lcond
from . import mol
from . import sampling
from . import train_pass

CH = 32
_EXPIRED = dict(
    coop='wn_fastgen_run_wide: a hand-over wait inside the cooperative '
         'generation launch expired (2 s: its workgroups were not all '
         'resident); state restored, continuing with the single workgroup '
         '(net.fastgen_wide_coop = False selects it up front)',
    persist='wn_fastgen_persist: a hand-over wait inside the persistent '
            'generation launch expired (2 s: its workgroups were not all '
            'resident); state restored, continuing with the step kernels '
            '(net.fastgen_persistent = False selects them up front)')


# ------------------------------------------------ shared by both generators
def _new_state(net, dil, nfl, rows, nbias, **extra):
    # queues of nfl floats, bias of nbias streams, step scratch of `rows`
    f32 = dict(dtype=torch.float32, device=net.device)
    return dict(
        state=torch.zeros(nfl, **f32),
        # one stream: [0] steps done, [1] previous code, [2] draw pending;
        # B streams: [0] steps pushed, [1] draw pending
        cursors=torch.zeros(4, dtype=torch.int32, device=net.device),
        dil=torch.from_numpy(dil).to(net.device),
        bias=torch.zeros(net.L * nbias * 2 * net.CHn, **f32),
        bsum=torch.zeros(net.S, **f32),
        ctl=torch.zeros(8, dtype=torch.int32, device=net.device),
        pre=torch.zeros(net.L * rows * 2 * CH, **f32),
        z_all=torch.zeros(rows * net.L * CH, **f32),
        h1=torch.zeros(rows * net.S, **f32),
        h2=torch.zeros(rows * net.S, **f32),
        logits=torch.zeros(rows * net.Q, **f32),
        graphs={}, warm=False, steps=0, **extra)


# ----------------------------------------------- local conditioning (LC)
# A call of n_steps steps on an LC model runs in chunks of C steps.  Before
# the chunk at call step a, the conditioned-bias ring (wn_fastgen_lc_bias)
# gets the rows of steps a .. a + C: step t also forms step t + 1's past-tap
# pre-activations, so a chunk needs one row past its end and the ring
# R = C + 1 rows (slot = position % R).  The row past the call's last input is
# written from a zero LC row; its value is never used, since every call
# recomputes its first step's pre-activations.
LC_RING_BYTES = 256 << 20
# one stream: a smaller ring (it stays allocated with the generator); 2600
# steps per chunk for the default stack, one persistent launch each
LC_RING_BYTES_ONE = 32 << 20


def lc_chunk(n_steps, row_bytes, forced=None, graph_steps=200, proba_every=1,
             budget=LC_RING_BYTES):
    """Steps per chunk: `forced` (net.fastgen_lc_chunk), else as many as a
    ring of `budget` bytes holds (rows of `row_bytes`) rounded down to a
    multiple of the graph length, but at least one graph length; then a
    multiple of proba_every (so that every chunk starts on a probability
    row) and at most n_steps."""
    if forced is not None:
        c = int(forced)
        if c < 1:
            raise ValueError('fastgen_lc_chunk must be >= 1 or None, got %r'
                             % (forced,))
    else:
        c = max(1, int(budget) // int(row_bytes) - 1)
        c = max(int(graph_steps), c - c % int(graph_steps))
    pe = max(1, int(proba_every))
    c = -(-c // pe) * pe
    return max(1, min(c, int(n_steps)))


def lc_plan(n_steps, chunk):
    """[(a, n)]: chunks of n steps starting at call step a; each fills ring
    rows a .. a + n (n + 1 rows; row n_steps is the zero lookahead row)."""
    return [(a, min(chunk, n_steps - a)) for a in range(0, n_steps, chunk)]


def _lc_device(net, lc):
    # a call's LC rows, checked by the model, as float32 on the device (once)
    return None if lc is None else lc.to(device=net.device,
                                         dtype=torch.float32).contiguous()


def _lc_rows_padded(net, lc, n_steps):
    # [..., n_steps, Lc] -> float32 [..., n_steps + 1, Lc] (the zero row)
    z = torch.zeros(lc.shape[:-2] + (1, net.Lc), dtype=torch.float32,
                    device=net.device)
    return torch.cat([lc.to(device=net.device, dtype=torch.float32), z],
                     dim=-2).contiguous()


class _LcRing(object):
    """The ring of one call: rows of `lcz` [nl, n_steps + 1, Lc] (nl = 1:
    shared by all B streams) for the positions p0 + call step."""

    def __init__(self, net, g, lcz, B, bias, bstride, n_steps, pe):
        self.net, self.lcz, self.B = net, lcz, B
        self.bias, self.bstride = bias, bstride
        self.lc_stride = lcz.shape[-2] * net.Lc if lcz.shape[0] > 1 else 0
        self.rstride = 64 if (self.lc_stride or bstride) else 0
        nr = B if self.rstride else 1
        row = net.L * nr * 64
        # (g['reserve']: the longest call of a run whose calls share graphs)
        self.C = lc_chunk(max(n_steps, g.get('reserve', 0)), row * 4,
                          net.fastgen_lc_chunk,
                          int(net.fastgen_graph_steps), pe,
                          LC_RING_BYTES if B > 1 else LC_RING_BYTES_ONE)
        self.R = self.C + 1
        self.ring = _buf(net, g, 'lc_ring', self.R * row, torch.float32)
        self.args = (_lib.ptr(self.ring), self.R, self.rstride)
        self.p0 = int(g['steps'])
        self.plan = lc_plan(n_steps, self.C)

    def fill(self, a, n):
        net = self.net
        _lib.call('wn_fastgen_lc_bias', _lib.ptr(self.lcz[0, a]),
                  self.lc_stride, net.Lc, _lib.ptr(net._seg(net.params, 'lc_w')),
                  net.L, self.bias, self.bstride, self.B,
                  self.p0 + a, n + 1, _lib.ptr(self.ring), self.R,
                  self.rstride, _lib.stream())


def _check_temperature(temperature):
    if not (np.isfinite(float(temperature)) and float(temperature) > 0.0):
        raise ValueError('temperature must be a finite number > 0, got %r'
                         % (temperature,))


# Top-k / nucleus truncation of the draw (wavenet/sampling.py has the rule):
# `trunc` = (top_k, top_p) as sampling.resolve gives them, 0 meaning off.  The
# step, persistent and batched launches read them from ctl words 6, 7 (as the
# temperature: captured graphs stay valid); the entry points with a scalar
# temperature have _trunc counterparts, called only when one of them is on.
_NO_TRUNC = (0, 0.0)


def _entry(name, lc=(), trunc=_NO_TRUNC, q=()):
    """(entry point, its arguments in front of the stream): `name` with the
    ABI's suffix for every argument group that is there (lc: a ring's args,
    trunc with one of the two on, q: the restarted streams' origins) and the
    groups in the ABI's order."""
    t = (int(trunc[0]), float(trunc[1])) if trunc != _NO_TRUNC else ()
    return (name + '_lc' * bool(lc) + '_trunc' * bool(t) + '_q' * bool(q),
            tuple(lc) + t + tuple(q))


def _buf(net, g, name, n, dtype):
    """Persistent buffer of g of at least n elements (grown geometrically;
    growing drops the captured graphs, which hold its address)."""
    buf = g.get(name)
    if buf is None or buf.numel() < n:
        cap = max(int(n), 2 * (buf.numel() if buf is not None else 0), 4096)
        g[name] = buf = torch.zeros(cap, dtype=dtype, device=net.device)
        g['graphs'].clear()
    return buf


def _weights(net, g, gc, B):
    """GC / filter-gate bias and skip-bias sum of B streams -> the nine
    parameter pointers, the bias pointer and its stream stride."""
    P, ub = net.params, net.use_biases
    bias, bstride = train_pass.bias_fg(net, g['bias'],
                                       net._gc_ids(gc, B), B)
    bsum = None
    if ub:
        _lib.call('wn_sum_rows', _lib.ptr(net._seg(P, 'skip_b')), net.L,
                  net.S, _lib.ptr(g['bsum']), _lib.stream())
        bsum = g['bsum']
    w = (_lib.ptr(net._seg(P, 'causal')), _lib.ptr(net._layer_block(P, 0)),
         net.layer_stride, _lib.ptr(net._seg(P, 'skip_w')), _lib.ptr(bsum),
         _lib.ptr(net._seg(P, 'post1_w')),
         _lib.ptr(net._seg(P, 'post1_b')) if ub else None,
         _lib.ptr(net._seg(P, 'post2_w')),
         _lib.ptr(net._seg(P, 'post2_b')) if ub else None)
    return w, _lib.ptr(bias), bstride


def _stage(net, g, io, n_given, n_steps, temperature, proba, proba_every,
           seed=None, trunc=_NO_TRUNC):
    # per-call values go to ctl and two persistent buffers (codes io [B, >=
    # n_steps + 1], probabilities), so captured graphs stay valid; ctl words
    # 4-5: one stream's seed, or B streams' row stride and probability rows;
    # 6-7: top_k and top_p of the draw
    B, ld = io.shape[0], int(n_steps) + 1
    pe = max(1, int(proba_every))
    rows = (int(n_steps) + pe - 1) // pe if proba is not None else 0
    iob = _buf(net, g, 'io_buf', B * max(ld, g.get('reserve', 0) + 1),
               torch.int32)
    iob[:B * ld].view(B, ld).copy_(io[:, :ld])
    pb = None
    if proba is not None:
        pb = _buf(net, g, 'proba_buf', B * rows * net.Q, torch.float32)
    ctl = np.zeros(8, np.uint32)
    ctl[0], ctl[1], ctl[2] = g['steps'], int(n_given), pe
    ctl[3] = np.float32(temperature).view(np.uint32)
    ctl[4], ctl[5] = (ld, rows) if seed is None else \
        (seed & 0xffffffff, seed >> 32)
    ctl[6], ctl[7] = trunc[0], np.float32(trunc[1]).view(np.uint32)
    g['ctl'].copy_(torch.from_numpy(ctl.view(np.int32)))
    return iob, pb


def _replay_steps(net, g, key, one, n_steps):
    """n_steps calls of one() (a step's launches) for generator dict g:
    the first step g ever runs outside any capture, then hipGraphs of
    fastgen_graph_steps and of a tenth of that many steps, captured once
    per (key, length) and replayed, then single steps.  key must hold
    every pointer and value the launches were given."""
    def graph_of(nsteps):
        gr = g['graphs'].get((key, nsteps))
        if gr is None:
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for _ in range(nsteps):
                    one()
            if len(g['graphs']) > 8:
                g['graphs'].clear()
            g['graphs'][key, nsteps] = gr
        return gr
    done = 0
    if not g['warm']:
        one()                      # module load etc. outside any capture
        done, g['warm'] = 1, True
    for per in (int(net.fastgen_graph_steps),
                max(1, int(net.fastgen_graph_steps) // 10)):
        if per > 1 and n_steps - done >= per:
            gr = graph_of(per)
            while n_steps - done >= per:
                gr.replay()
                done += per
    for _ in range(n_steps - done):
        one()


def _expired(net, kind, scratch, restore):
    # what the residency check cannot see (CUs held elsewhere, a CU mask)
    # shows as an expired hand-over wait, word 12 of the scratch: `restore`
    # is copied back and the caller repeats the run on a path that always
    # completes.  (synchronises; a generation call ends on the host anyway)
    if int(scratch[12]) == 0:
        return False
    warnings.warn(_EXPIRED[kind])
    for t, saved in restore:
        t.copy_(saved)
    # (remembered on the MODEL: a new generator on the same busy device must
    # not pay another expired wait)
    net._gen_launch_failed[kind] = True
    return True


def _prime(net, g, n0, groups, Bp):
    # ONE batch-1 forward pass per (codes [n0], GC id, streams): layer l's
    # queue holds its last d_l inputs x_l[t] (model.py:473-484), rows of
    # activation planes l * CB + cb; ring rows are [entries][Bp][32]
    CB = net.CB
    src, dst, roff = [], [], 0
    for l, d in enumerate(net.dilations):
        t = np.arange(max(0, n0 - d), n0, dtype=np.int64)
        for cb in range(CB):
            src.append((l * CB + cb) * n0 + t)
            dst.append((roff + t % d) * CB + cb)
        roff += d
    src = torch.from_numpy(np.concatenate(src)).to(net.device)
    dst = np.concatenate(dst)
    ws = net._workspace(1, n0, False)
    for codes, gc, streams, lc in groups:
        if net.mol_K:
            # (levels: the network reads their centres, as in training)
            mol.stage(net, ws, torch.from_numpy(mol.centres(
                codes.numpy())).to(net.device).reshape(1, n0), None)
        else:
            ws.q.copy_(codes)
        lcond.fill(net, lc, ws)    # the seed's LC rows, as predict_proba
        train_pass.run_pass(net, 'fwd', ws, net._gc_ids(gc, 1),
                            train_pass.step_path(net, ws, False))
        # (+ the forward launch's poison word: 0, or NaN after an expired wait)
        vals = ws.X.reshape(-1, CH).index_select(0, src) + ws.loss_parts[0]
        rows = dst[None, :] * Bp + np.asarray(streams, np.int64)[:, None]
        g['state'].view(-1, CH).index_copy_(
            0, torch.from_numpy(rows.reshape(-1)).to(net.device),
            vals.repeat(len(streams), 1))


def _seeded(net, io, n_given, n, pe, prime, run, lc=None, row=None):
    # io [..., n_given + n] starts with the seed codes; returns the
    # probabilities [..., rows, Q] of every pe-th step, or None.  lc: the
    # call's LC rows [..., n_steps, Lc] (run gets those of its steps); row:
    # the shape of a returned row where it is not (Q,)
    n_steps = n_given - 1 + n
    primed = prime and pe == 0 and \
        n_given - 1 >= net.fastgen_prime_forward_min and n > 0 and \
        (lc is None or lcond.forward_ok(net, n_given - 1))
    if lc is not None:
        run = functools.partial(run, lc=lc[..., n_given - 1:, :] if primed
                                else lc)
    proba = None
    if pe > 0:
        proba = torch.empty(io.shape[:-1] + ((n_steps + pe - 1) // pe,) +
                            tuple(row or (net.Q,)),
                            dtype=torch.float32, device=net.device)
    if primed:
        # the reference's own TODO (generate.py:199-201): fill the queues
        # from a forward pass over the seed instead of stepping through it
        prime()
        tail = io[..., n_given - 1:].clone()   # [last seed | generated ...]
        run(tail, 1, n, None, 1)
        io[..., n_given - 1:] = tail
    elif n_steps > 0:
        run(io, n_given, n_steps, proba, max(1, pe))
    return proba


# --------------------------------------------------------------- one stream
def generator(net, global_condition):
    """Device-resident incremental-generation state (_create_generator,
    model.py:444-516): ring buffers standing in for the FIFO queues."""
    if net.CHn > net.FASTGEN_MAX_CHANNELS:
        raise NotImplementedError(
            'fast (incremental) generation supports at most %d residual / '
            'dilation channels on the HIP path; predict_proba (generate.py '
            'without --fast_generation) has no such limit'
            % net.FASTGEN_MAX_CHANNELS)
    if net._gen is None:
        dil = np.asarray(net.dilations, dtype=np.int32)
        # (queue entries are rows of CHn = 32 * blocks floats)
        nfl = _lib.load().wn_fastgen_state_floats(dil.ctypes.data,
                                                  net.L) * net.CB
        f32 = dict(dtype=torch.float32, device=net.device)
        net._gen = _new_state(
            net, dil, nfl, 1, 1, cw_img=torch.zeros(net.L * 3072, **f32),
            proba=torch.empty(net.Q, **f32),
            io=torch.zeros(2, dtype=torch.int32, device=net.device))
        reset(net)
    return net._gen


def reset(net):
    g = net._gen
    _lib.call('wn_fastgen_init', _lib.ptr(g['state']), g['state'].numel(),
              _lib.ptr(g['cursors']), net.L, _lib.stream())
    g['steps'] = 0


def run(net, temperature, seed, global_condition, samples_io, n_given,
        n_steps, proba_out, proba_every, push=True, multi_cu=False, lc=None,
        trunc=_NO_TRUNC):
    """Run `n_steps` generation steps on samples_io int32 [n_steps + 1]
    (the first n_given codes given, the rest drawn) on one device path.
    lc: an LC model's rows [n_steps, Lc], row i beside samples_io[i].
    trunc: (top_k, top_p) of sampling.resolve."""
    # (wn_fastgen_step reads both from the device control block and cannot
    # reject them; the reference applies the temperature as log(p) / T,
    # generate.py:229-233)
    _check_temperature(temperature)
    if int(n_given) < 1:
        raise ValueError('n_given must be >= 1, got %r' % (n_given,))
    g = generator(net, global_condition)
    w, bias, _ = _weights(net, g, global_condition, 1)
    head = w + (bias, _lib.ptr(g['dil']))
    queues = (_lib.ptr(g['state']), _lib.ptr(g['cursors']))
    n_given, n_steps = int(n_given), int(n_steps)
    temperature, sd = float(temperature), int(seed) & (2**64 - 1)
    # (every caller's proba_every is >= 1)
    pe, ub = max(1, int(proba_every)), 1 if net.use_biases else 0
    if lc is None and (net.CB > 1 or net.S > 512 or net.Q > 512 or net.L > 64):
        _run_wide(net, g, samples_io,
                  head + (net.L, net.CHn, net.S, net.Q) + queues +
                  (_lib.ptr(samples_io), n_given, n_steps, temperature, sd,
                   _lib.ptr(proba_out), pe, ub, 1 if push else 0), trunc)
    else:
        _run_chunks(net, g, head + (net.L, net.S, net.Q) + queues, bias,
                    samples_io, n_given, n_steps, temperature, sd, proba_out,
                    pe, ub, push, multi_cu, lc, trunc)
    if push:
        g['steps'] += n_steps


def _run_chunks(net, g, head, bias, samples_io, n_given, n_steps, temperature,
                sd, proba_out, pe, ub, push, multi_cu, lc, trunc):
    # One call of the 32-channel kernels (head: the arguments up to the
    # queues), chunk by chunk: an LC call has its ring's plan and arguments
    # (see _LcRing), a plain call is one chunk with neither.
    plan, lcargs, fill = [(0, n_steps)], (), lambda a, n: None
    if lc is not None:
        ring = _LcRing(net, g, _lc_rows_padded(
            net, lc.reshape(1, n_steps, net.Lc), n_steps), 1, bias, 0,
            n_steps, pe)
        plan, lcargs, fill = ring.plan, ring.args, ring.fill

    def prows(a):                  # the probability rows from call step a
        return None if proba_out is None else \
            proba_out.view(-1)[a // pe * net.Q:]
    if not multi_cu or not push:
        # ONE single-workgroup kernel a chunk; the peek always runs here, as
        # the multi-CU launches advance the queues with every step they take
        name, extra = _entry('wn_fastgen_run', lcargs, trunc)
        for a, n in plan:
            fill(a, n)
            _lib.call(name, *head, _lib.ptr(samples_io[a:]),
                      max(1, n_given - a), n, temperature, sd,
                      _lib.ptr(prows(a)), pe, ub, 1 if push else 0, *extra,
                      _lib.stream())
        return
    st = _lib.stream()
    layer0 = _lib.ptr(net._layer_block(net.params, 0))
    # weights are constant while generating: pack the chain blocks once
    _lib.call('wn_fastgen_pack', layer0, net.layer_stride,
              _lib.ptr(g['cw_img']), net.L, st)
    io = samples_io.view(1, -1)
    steps0 = g['steps']

    def stage(a, n_fill, n_run):
        # ring rows of n_fill steps from a, the past-tap pre-activations of
        # step a (every step then leaves the next step's behind), and steps
        # a .. a + n_run staged as a call of their own (ctl, io, proba)
        fill(a, n_fill)
        _lib.call(_entry('wn_fastgen_pre', lcargs)[0], layer0,
                  net.layer_stride, bias, _lib.ptr(g['dil']), net.L,
                  _lib.ptr(g['state']), _lib.ptr(g['cursors']),
                  _lib.ptr(g['pre']), *lcargs, st)
        g['steps'] = steps0 + a
        pr = prows(a)
        iob, pb = _stage(net, g, io[:, a:], max(1, n_given - a), n_run,
                         temperature, pr, pe, seed=sd, trunc=trunc)
        args = head + (
            _lib.ptr(iob), _lib.ptr(g['ctl']), _lib.ptr(pb), ub,
            _lib.ptr(g['cw_img']), _lib.ptr(g['pre']), _lib.ptr(g['z_all']),
            _lib.ptr(g['h1']), _lib.ptr(g['h2']), _lib.ptr(g['logits']))

        def done():
            samples_io[a:a + n_run + 1].copy_(iob[:n_run + 1])
            if pr is not None:
                k = (n_run + pe - 1) // pe * net.Q
                pr[:k].copy_(pb[:k])
        return iob, pb, args, done
    a_step, staged = 0, None       # where the step kernels take over
    if net.fastgen_persistent and not net._gen_launch_failed.get('persist'):
        for a, n in plan:
            staged = iob, pb, args, done = stage(a, n, n)
            if not _run_persistent(net, g, args, io[:, a:], iob, n, lcargs):
                break
            done()
            a_step = a + n
    if a_step < n_steps:
        # the step kernels from call step a_step (state as the launches left
        # it), staged as ONE call, an LC call's ring refilled chunk by chunk.
        # (A plain call's refused launch was staged as just that.)
        plan = [(a, n) for a, n in plan if a >= a_step]
        if lcargs or staged is None:
            staged = stage(a_step, plan[0][1], n_steps - a_step)
        iob, pb, args, done = staged
        name = _entry('wn_fastgen_step', lcargs)[0]
        for i, (a, n) in enumerate(plan):
            if i:
                fill(a, n)
            # (the stream is looked up inside: a capture runs on its own)
            _replay_steps(net, g, (args, lcargs), lambda: _lib.call(
                name, *args, *lcargs, _lib.stream()), n)
        # the last step's draw (every other one ran inside the next step)
        _lib.call('wn_fastgen_finish', net.Q, _lib.ptr(g['cursors']),
                  _lib.ptr(iob), _lib.ptr(g['ctl']), _lib.ptr(pb),
                  _lib.ptr(g['logits']), st)
        done()
    g['steps'] = steps0


def _run_wide(net, g, samples_io, args, trunc=_NO_TRUNC):
    # more than 32 channels, or more S / Q / L than the tuned kernels hold
    # in LDS: one workgroup, or the cooperative launch (skip sum and post-
    # processing on other CUs) where the library has one for the shape
    name, targs = _entry('wn_fastgen_run_wide', trunc=trunc)
    coop = None
    if net.fastgen_wide_coop and not net._gen_launch_failed.get('coop'):
        if 'coop' not in g:
            nb = _lib.load().wn_fastgen_wide_coop_bytes(
                net.L, net.CHn, net.S, net.Q)
            g['coop'] = torch.zeros(nb // 4, dtype=torch.int32,
                                    device=net.device) if nb else None
        coop = g['coop']
    if coop is not None:
        # an expired wait: queues, cursors and samples are restored and the
        # single workgroup, which always completes, repeats the run
        snap = [(t, t.clone()) for t in (g['state'], g['cursors'], samples_io)]
        _lib.call(name, *args, _lib.ptr(coop), *targs, _lib.stream())
        if not _expired(net, 'coop', coop, snap):
            return
    _lib.call(name, *args, None, *targs, _lib.stream())


def _run_persistent(net, g, args, io, iob, n_steps, lcargs):
    # ONE launch for the run; its workgroups must all be resident, which
    # the library checks (WN_ERR_UNSUPPORTED).  False: the step kernels, which
    # always complete, run it (after an expired wait, from restored state)
    lib = _lib.load()
    name, extra = _entry('wn_fastgen_persist', lcargs)
    sync = _buf(net, g, 'fgp_sync', 16, torch.int32)
    ll = _buf(net, g, 'fgp_ll', int(lib.wn_fastgen_persist_ll_words(
        net.L, net.S, net.Q)), torch.int64)
    snap = [(t, t.clone()) for t in (g['state'], g['cursors'], g['pre'])]
    # (the library's attribute as it is now; the error code is read here)
    code = getattr(lib, name)(*args, _lib.ptr(sync), _lib.ptr(ll),
                              int(n_steps), *extra, _lib.stream())
    if code == 0:
        n_io = int(n_steps) + 1
        return not _expired(net, 'persist', sync,
                            snap + [(iob[:n_io], io[0, :n_io])])
    if code != -2:                 # WN_ERR_UNSUPPORTED: not resident / shape
        _lib.check(code, name)
    return False


def _follow_up(net):
    """What a refusal of a scalar_input (softmax or mixture head) model
    adds: fast generation for it is planned, not impossible."""
    return '; ' + mol.FOLLOW_UP if net.scalar_input else ''


def predict_proba_incremental(net, waveform, global_condition, push, lc=None):
    if net.filter_width > 2:
        raise NotImplementedError("Incremental generation does not "
                                  "support filter_width > 2.")
    if net.scalar_input:
        raise NotImplementedError("Scalar input is not supported by "
                                  "fast generation yet: " + mol.FOLLOW_UP)
    net._check_supported()
    g = generator(net, global_condition)
    w = waveform
    if isinstance(w, torch.Tensor):
        g['io'][0:1].copy_(w.reshape(-1)[-1:].to(torch.int32))
    else:
        g['io'][0] = int(np.asarray(w).reshape(-1)[-1])
    run(net, 1.0, 0, global_condition, g['io'], 1, 1, g['proba'], 1,
        push=push, lc=lc)
    return g['proba'].clone()


def generate(net, num_samples, seed_samples, temperature, global_condition,
             seed, return_proba_every, lc=None, top_k=None, top_p=None):
    trunc = sampling.resolve(top_k, top_p, net.Q)
    if net.filter_width > 2 or net.scalar_input:
        raise NotImplementedError('fast generation needs filter_width 2 '
                                  'and one-hot input (model.py:597-603)'
                                  + _follow_up(net))
    net._check_supported()
    lc = _lc_device(net, lc)
    if seed_samples is None:
        seed_samples = [net.Q // 2]
    s = torch.as_tensor(np.asarray(seed_samples),
                        dtype=torch.int32).reshape(-1)
    n_given, n = int(s.numel()), int(num_samples)
    io = torch.zeros(n_given + n, dtype=torch.int32, device=net.device)
    io[:n_given] = s.to(net.device)
    # (net.reset_generator(), which an LC model refuses)
    generator(net, None)
    reset(net)
    pe = int(return_proba_every)
    proba = _seeded(net, io, n_given, n, pe,
                    lambda: prime(net, io[:n_given - 1], global_condition,
                                  None if lc is None else lc[:n_given - 1]),
                    functools.partial(run, net, temperature, seed,
                                      global_condition,
                                      multi_cu=net.fastgen_multi_cu,
                                      trunc=trunc), lc)
    return (io, proba) if pe > 0 else io


def prime(net, codes, global_condition, lc=None):
    if net.filter_width > 2 or net.scalar_input:
        raise NotImplementedError('fast generation needs filter_width 2 '
                                  'and one-hot input (model.py:597-603)'
                                  + _follow_up(net))
    net._check_supported()
    g = generator(net, global_condition)
    reset(net)
    lc = _lc_device(net, lc)
    w = torch.as_tensor(codes).to(device=net.device,
                                  dtype=torch.int32).reshape(-1)
    n0 = int(w.numel())
    if n0 == 0:
        return
    _prime(net, g, n0, [(w, global_condition, [0], lc)], 1)
    g['cursors'][0] = n0
    g['cursors'][1:2].copy_(w[-1:])
    g['steps'] = n0


def continue_generation(net, num_samples, last_sample, temperature,
                        global_condition, seed, lc=None, top_k=None,
                        top_p=None):
    trunc = sampling.resolve(top_k, top_p, net.Q)
    net._check_supported()
    n = int(num_samples)
    io = torch.zeros(n + 1, dtype=torch.int32, device=net.device)
    io[0] = int(last_sample)
    run(net, temperature, seed, global_condition, io, 1, n, None, 1,
        multi_cu=net.fastgen_multi_cu, lc=lc, trunc=trunc)
    return io[1:]


# ---------------------------------------------------------------- B streams
def _batch_args(net, seeds, per_stream, global_condition, temperature,
                num_samples, mixture=False):
    """The batched entry points' checks, in order, before anything touches
    a device -> seeds (int64 bit patterns), per_stream(B), GC ids, n.
    mixture: the generate_mixture_batch path, where scalar input is the
    input (initial_filter_width <= 32) and temperature 0 is legal; its
    refusals name that call and the naive path, the only other one."""
    what = 'generate_mixture_batch' if mixture else 'generate_batch'
    other = 'predict_mixture (generate.py --fast_generation false)' \
        if mixture else 'generate() per stream'
    if net.CB > 1:
        raise NotImplementedError(
            '%s supports at most 32 residual / dilation '
            'channels (this model has %d); use %s'
            % (what, max(net.R, net.D), other))
    if mixture:
        if net.filter_width > 2:
            raise NotImplementedError(
                'generate_mixture_batch needs filter_width 2, as every fast '
                'generation path does; use predict_mixture (generate.py '
                '--fast_generation false)')
        if net.initial_filter_width > MOL_MAX_INITIAL_WIDTH:
            raise NotImplementedError(
                'generate_mixture_batch supports initial_filter_width 1 to '
                '%d (the 64-slot level history), this model has %d; use '
                'predict_mixture (generate.py --fast_generation false)'
                % (MOL_MAX_INITIAL_WIDTH, net.initial_filter_width))
    elif net.filter_width > 2 or net.scalar_input:
        raise NotImplementedError(
            'generate_batch needs filter_width 2 and one-hot input '
            '(model.py:597-603), as every fast generation path does; use '
            'predict_proba (generate.py --fast_generation false)'
            + _follow_up(net))
    if net.S > 512 or net.Q > 512 or net.L > 64:
        raise NotImplementedError(
            '%s supports at most 512 skip / quantization '
            'channels and 64 layers; use %s' % (what, other))
    s = [int(v) & (2**64 - 1) for v in seeds]
    if not 1 <= len(s) <= net.FASTGEN_BATCH_MAX:
        raise ValueError('%s takes 1 to %d streams (one seed '
                         'each), got %d' % (what, net.FASTGEN_BATCH_MAX,
                                            len(s)))
    B = len(s)
    rows = per_stream(B)
    gc = global_condition
    if gc is not None:
        if isinstance(gc, torch.Tensor):
            gc = gc.cpu().numpy()
        gc = np.asarray(gc).reshape(-1)
        if gc.size == 1:
            gc = np.repeat(gc, B)
        if gc.size != B:
            raise ValueError('global_condition has %d ids for %d streams'
                             % (gc.size, B))
        gc = gc.astype(np.int32)
    if mixture:
        if not (np.isfinite(float(temperature)) and
                float(temperature) >= 0.0):
            raise ValueError('temperature must be a finite number >= 0, got '
                             '%r' % (temperature,))
    else:
        _check_temperature(temperature)
    n = int(num_samples)
    if n < 0:
        raise ValueError('num_samples must be >= 0, got %d' % n)
    net._check_supported()
    return np.asarray(s, dtype=np.uint64).view(np.int64), rows, gc, n


def _batch_codes(net, seed_samples, B):
    """seed_samples -> int32 [B, n]: None (Q // 2 for every stream), one
    sequence shared by all streams, or one row per stream."""
    if seed_samples is None:
        return np.full((B, 1), net.Q // 2, np.int32)
    if isinstance(seed_samples, torch.Tensor):
        seed_samples = seed_samples.cpu().numpy()
    try:
        a = np.asarray(seed_samples)
    except ValueError:             # ragged rows
        a = None
    if a is None or a.dtype == object or a.ndim not in (1, 2):
        raise ValueError('seed_samples must be None, one sequence shared '
                         'by all streams, or [B, n]: the same number of '
                         'seed codes for every stream')
    if a.ndim == 1:
        a = np.broadcast_to(a, (B, a.shape[0]))
    if a.shape[0] != B:
        raise ValueError('seed_samples has %d rows for %d streams'
                         % (a.shape[0], B))
    if a.shape[1] < 1:
        raise ValueError('seed_samples needs at least one code per stream')
    return np.array(a, dtype=np.int32, order='C')   # (a writable copy)


def _batch_last(last, B):
    if isinstance(last, torch.Tensor) and last.is_cuda:
        # (stays on the device: nothing waits for the codes of the call before)
        if last.numel() != B:
            raise ValueError('last_samples has %d codes for %d streams'
                             % (last.numel(), B))
        return last.reshape(-1).to(torch.int32)
    if isinstance(last, torch.Tensor):
        last = last.cpu().numpy()
    last = np.asarray(last, dtype=np.int32).reshape(-1)
    if last.size != B:
        raise ValueError('last_samples has %d codes for %d streams'
                         % (last.size, B))
    return last


def _batch_restart_arg(restart, B):
    """restart -> None or a sorted list of stream indices: ints in [0, B),
    no duplicates (ValueError before the library or a device is touched)."""
    if restart is None:
        return None
    if isinstance(restart, torch.Tensor):
        restart = restart.cpu().numpy()
    a = np.asarray(restart)
    if a.ndim == 1 and a.size == 0:
        return None
    if a.ndim != 1 or a.dtype == np.bool_ or \
            not np.issubdtype(a.dtype, np.integer):
        raise ValueError('restart must be None or a list of stream indices '
                         '(ints), got %r' % (restart,))
    a = a.astype(np.int64)
    if a.min() < 0 or a.max() >= B or np.unique(a).size != a.size:
        raise ValueError('restart must name distinct streams in [0, %d), '
                         'got %r' % (B, a.tolist()))
    return sorted(int(v) for v in a)


def batch_generator(net, B):
    """Device state of the batched generator for B streams, separate from
    the single-stream generator's (`_gen`): ring rows [sum d][Bp][32]."""
    g = net._bgen
    if g is not None and g['B'] == B:
        return g
    net._bgen = None
    lib = _lib.load()
    Bp = lib.wn_fastgen_batch_rows(B)
    _lib.check(min(Bp, 0), 'wn_fastgen_batch_rows')
    dil = np.asarray(net.dilations, dtype=np.int32)
    nfl = lib.wn_fastgen_batch_state_floats(dil.ctypes.data, net.L, B)
    _lib.check(int(min(nfl, 0)), 'wn_fastgen_batch_state_floats')
    net._bgen = _new_state(
        net, dil, nfl, Bp, B, B=B, Bp=Bp,
        seeds=torch.zeros(B, dtype=torch.int64, device=net.device),
        prev=torch.full((Bp,), -1, dtype=torch.int32, device=net.device),
        # the step at which each stream (re)started; `restarted`: some
        # origin may differ from 0, the _q entry points run
        origin=torch.zeros(Bp, dtype=torch.int32, device=net.device),
        flags=torch.zeros(Bp, dtype=torch.int32, device=net.device),
        restarted=False, reserve=0)
    if net.mol_K:
        # levels input: slot T & 63 holds the level consumed at step T
        net._bgen['hist'] = torch.full((Bp, MOL_HIST), -1, dtype=torch.int32,
                                       device=net.device)
    return net._bgen


def batch_reset(net, g):
    _lib.call('wn_fastgen_batch_init', _lib.ptr(g['state']),
              g['state'].numel(), _lib.ptr(g['cursors']),
              _lib.ptr(g['prev']), g['B'], _lib.stream())
    g['steps'] = 0
    if g['restarted']:
        g['origin'].zero_()
        g['restarted'] = False


def batch_restart(net, g, streams):
    """Make the streams `streams` fresh ones at the step the queues are at
    (wn_fastgen_batch_restart: zero queues, no previous code, the draw
    counted from here).  Between two calls only: no draw is pending."""
    flags = np.zeros(g['Bp'], np.int32)
    flags[streams] = 1
    g['flags'].copy_(torch.from_numpy(flags))
    _lib.call('wn_fastgen_batch_restart', _lib.ptr(g['state']),
              _lib.ptr(g['dil']), net.L, g['B'], _lib.ptr(g['cursors']),
              _lib.ptr(g['prev']), _lib.ptr(g['origin']),
              _lib.ptr(g['flags']), _lib.stream())
    g['restarted'] = True


def batch_lc_rows(net, items, pos0, n):
    """float32 [B, n, Lc] on the device, the LC rows of the n lock-step steps
    from position pos0 for B streams that hold different items
    (wn_fastgen_batch_lc_rows).  items[b]: None, or (rows, origin): rows a
    float32 device tensor [m, Lc] (contiguous), origin the step at which
    the stream's item started.  The stream's own step t = pos0 + j - origin
    gets rows[t - 1] for 1 <= t <= m, zeros elsewhere."""
    B, Lc = len(items), int(net.Lc)
    table = np.zeros((B, 3), np.int64)
    for b, it in enumerate(items):
        if it is None or it[0] is None or int(it[0].shape[0]) == 0:
            continue
        rows, origin = it
        if rows.dtype != torch.float32 or not rows.is_contiguous() or \
                rows.dim() != 2 or int(rows.shape[1]) != Lc or \
                not rows.is_cuda:
            raise ValueError('batch_lc_rows: rows of stream %d must be a '
                             'contiguous float32 [m, %d] on the device'
                             % (b, Lc))
        table[b] = rows.data_ptr(), int(origin), int(rows.shape[0])
    out = torch.empty((B, int(n), Lc), dtype=torch.float32, device=net.device)
    tb = torch.from_numpy(table).to(net.device)
    _lib.call('wn_fastgen_batch_lc_rows', _lib.ptr(tb), B, int(n), Lc,
              int(pos0), _lib.ptr(out), _lib.stream())
    return out


def batch_prepare(net, g, io, n_given, n_steps, temperature, seeds, proba,
                  proba_every, gc, lc=None, trunc=_NO_TRUNC):
    """Everything n_steps batched steps need before the first: the args of
    wn_fastgen_batch_step (no stream) and the buffers batch_complete reads.
    lc (LC models): rows [B or 1, n_steps, Lc]; the result then holds the
    call's ring (`ring`), its first chunk filled, and the pre-activations
    are those of wn_fastgen_batch_pre_lc.  `step` and `finish` are (entry
    point, its arguments in front of the stream) for this model: the
    wn_fastgen_batch_* entries with their _lc / _q suffixes, or, for a
    mixture model, the wn_fastgen_mol_* entries, whose LC ring and origins
    are nullable arguments."""
    B, mixture = g['B'], bool(net.mol_K)
    w, bias, bstride = _weights(net, g, gc, B)
    ring = None
    if lc is not None:
        ring = _LcRing(net, g, _lc_rows_padded(net, lc, n_steps), B, bias,
                       bstride, n_steps, proba_every)
        ring.fill(*ring.plan[0])
    g['seeds'].copy_(torch.from_numpy(seeds))
    iob, pb = _stage(net, g, io, n_given, n_steps, temperature, proba,
                     proba_every, trunc=trunc)
    lcargs = () if ring is None else ring.args
    # restarted streams: the _q entries, the origins in front of the stream
    q = (_lib.ptr(g['origin']),) if g['restarted'] else ()
    # past-tap pre-activations of the first step (every step then leaves
    # the next step's behind)
    pre_args = (_lib.ptr(net._layer_block(net.params, 0)), net.layer_stride,
                bias, bstride, _lib.ptr(g['dil']), net.L, B,
                _lib.ptr(g['state']), _lib.ptr(g['cursors']),
                _lib.ptr(g['pre']))
    queues = (_lib.ptr(g['state']), _lib.ptr(g['cursors']))
    io_args = (_lib.ptr(iob), _lib.ptr(g['ctl']), _lib.ptr(g['seeds']),
               _lib.ptr(pb))
    scratch = (_lib.ptr(g['pre']), _lib.ptr(g['z_all']), _lib.ptr(g['h1']),
               _lib.ptr(g['h2']), _lib.ptr(g['logits']))
    shape = (bias, bstride, _lib.ptr(g['dil']), net.L, net.S)
    ub = 1 if net.use_biases else 0
    if mixture:
        K, lsm = net.mol_K, net.mol_log_scale_min
        tail = tuple(lcargs or (None, 0, 0)) + (q[0] if q else None,)
        _lib.call('wn_fastgen_mol_pre', *pre_args, *tail[:3], _lib.stream())
        args = (w[0], net.initial_filter_width) + w[1:] + shape + (K, B) + \
            queues + (_lib.ptr(g['hist']),) + io_args + (ub, lsm) + scratch
        step = ('wn_fastgen_mol_step', tail)
        finish = ('wn_fastgen_mol_finish', (K, lsm, B, queues[1]) + io_args +
                  (scratch[4], tail[3]))
    else:
        _lib.call(_entry('wn_fastgen_batch_pre', lcargs)[0], *pre_args,
                  *lcargs, _lib.stream())
        args = w + shape + (net.Q, B) + queues + (_lib.ptr(g['prev']),) + \
            io_args + (ub,) + scratch
        step = _entry('wn_fastgen_batch_step', lcargs, q=q)
        finish = (_entry('wn_fastgen_batch_finish', q=q)[0],
                  (net.Q, B, queues[1]) + io_args + (scratch[4],) + q)
    return dict(args=args, iob=iob, pb=pb, ring=ring, q=q, step=step,
                finish=finish)


def batch_complete(net, g, prep, io, proba, n_steps):
    """The last step's draw (every other one runs at the next step's
    start), then the codes / probabilities back into io / proba."""
    name, args = prep['finish']
    _lib.call(name, *args, _lib.stream())
    g['steps'] += int(n_steps)
    io.copy_(prep['iob'][:io.numel()].view(io.shape))
    if proba is not None:
        proba.view(-1).copy_(prep['pb'][:proba.numel()])


def _batch_run(net, g, temperature, seeds, gc, io, n_given, n_steps, proba,
               proba_every, lc=None, trunc=_NO_TRUNC):
    # n_steps lock-step steps of all B streams on io [B, n_steps + 1]: five
    # kernels per step, captured into a hipGraph once and replayed (LC: in
    # chunks, the ring filled before each)
    prep = batch_prepare(net, g, io, n_given, n_steps, temperature, seeds,
                         proba, proba_every, gc, lc, trunc)
    args, ring = prep['args'], prep['ring']
    name, extra = prep['step']
    for i, (a, n) in enumerate([(0, n_steps)] if ring is None else ring.plan):
        if i:
            ring.fill(a, n)
        # (the stream is looked up inside: a capture runs on its own)
        _replay_steps(net, g, (name, args, extra), lambda: _lib.call(
            name, *args, *extra, _lib.stream()), n)
    batch_complete(net, g, prep, io, proba, n_steps)


def _reserve_arg(reserve_steps):
    r = 0 if reserve_steps is None else reserve_steps
    if isinstance(r, (bool, np.bool_)) or \
            not isinstance(r, (int, np.integer)) or r < 0:
        raise ValueError('reserve_steps must be None or an int >= 0, got %r'
                         % (reserve_steps,))
    return int(r)


def generate_batch(net, num_samples, seeds, seed_samples, temperature,
                   global_condition, return_proba_every, lc=None, top_k=None,
                   top_p=None, reserve_steps=None):
    trunc = sampling.resolve(top_k, top_p, net.Q)
    reserve = _reserve_arg(reserve_steps)

    def per_stream(B):
        codes = _batch_codes(net, seed_samples, B)
        if not net.Lc and lc is None:
            return codes, None
        return codes, lcond.fastgen_rows(net, lc, 'generate_batch',
                                         codes.shape[1] + int(num_samples) - 1,
                                         B)
    sd, (codes, lc), gc, n = _batch_args(net, seeds, per_stream,
                                         global_condition, temperature,
                                         num_samples)
    B, n_given = codes.shape
    lc = _lc_device(net, lc)
    out = torch.zeros((B, n_given + n), dtype=torch.int32, device=net.device)
    out[:, :n_given] = torch.from_numpy(codes).to(net.device)
    g = batch_generator(net, B)
    batch_reset(net, g)
    g['reserve'] = reserve

    def prime():
        # ONE forward pass per distinct (seed, GC id): a stream's queues are
        # bitwise those it gets alone, whatever B
        batch_reset(net, g)
        n0, groups = n_given - 1, {}
        # (LC: the seed's rows are part of the key)
        lch = None if lc is None else lc[:, :n0].cpu().numpy()
        for b in range(B):
            key = (codes[b, :n0].tobytes(), None if gc is None else int(gc[b]),
                   None if lch is None else lch[b % len(lch)].tobytes())
            groups.setdefault(key, []).append(b)
        _prime(net, g, n0, [
            (torch.from_numpy(np.ascontiguousarray(codes[s[0], :n0])),
             None if gc is None else gc[s[0]:s[0] + 1], s,
             None if lc is None else lc[s[0] % lc.shape[0], :n0])
            for s in groups.values()], g['Bp'])
        g['cursors'][0] = n0
        g['prev'][:B].copy_(torch.from_numpy(codes[:, n0 - 1].copy()))
        g['steps'] = n0
    pe = int(return_proba_every)
    proba = _seeded(net, out, n_given, n, pe, prime, functools.partial(
        _batch_run, net, g, temperature, sd, gc, trunc=trunc), lc)
    return (out, proba) if pe > 0 else out


def continue_generation_batch(net, num_samples, last_samples, seeds,
                              temperature, global_condition,
                              return_proba_every, lc=None, top_k=None,
                              top_p=None, restart=None, reserve_steps=None):
    trunc = sampling.resolve(top_k, top_p, net.Q)
    reserve = _reserve_arg(reserve_steps)
    restart = _batch_restart_arg(restart, len(seeds))

    def per_stream(B):
        last = _batch_last(last_samples, B)
        if not net.Lc and lc is None:
            return last, None
        return last, lcond.fastgen_rows(net, lc, 'continue_generation_batch',
                                        int(num_samples), B)
    sd, (last, lc), gc, n = _batch_args(net, seeds, per_stream,
                                        global_condition, temperature,
                                        num_samples)
    B = len(sd)
    g = net._bgen
    if g is None or g['B'] != B:
        raise RuntimeError('no batched generation of %d streams to '
                           'continue: call generate_batch first' % B)
    lc = _lc_device(net, lc)
    io = torch.zeros((B, n + 1), dtype=torch.int32, device=net.device)
    io[:, 0] = last if isinstance(last, torch.Tensor) else \
        torch.from_numpy(last).to(net.device)
    g['reserve'] = reserve
    if restart:
        batch_restart(net, g, restart)
    pe = int(return_proba_every)
    proba = _seeded(net, io, 1, n, pe, None,
                    functools.partial(_batch_run, net, g, temperature, sd, gc,
                                      trunc=trunc), lc)
    return (io[:, 1:], proba) if pe > 0 else io[:, 1:]


# ------------------------------------------- B streams, mixture of logistics
# The batched generator with its two ends replaced (csrc/wn_fastgen_mol.hip,
# include/wavenet_fastgen_mol.h): the causal layer reads a 64-slot history of
# each stream's levels, the draw is the mixture's.  State, buffers, graphs,
# the LC ring, priming and restarts are the batched generator's (`net._bgen`).
MOL_HIST = 64
MOL_MAX_INITIAL_WIDTH = 32


def _mol_need(net, what, other):
    if not net.mol_K:
        raise ValueError('%s: this model was built without output_mixture; '
                         'use %s' % (what, other))


def _mol_levels(seed_levels, B):
    """seed_levels -> int32 [B, n]: None (level 32768 for every stream), one
    sequence shared by all streams, or one row per stream; levels 0 .. 65535."""
    if seed_levels is None:
        return np.full((B, 1), mol.LEVELS // 2, np.int32)
    if isinstance(seed_levels, torch.Tensor):
        seed_levels = seed_levels.cpu().numpy()
    try:
        a = np.asarray(seed_levels)
    except ValueError:             # ragged rows
        a = None
    if a is None or a.dtype == object or a.ndim not in (1, 2) or \
            not (np.issubdtype(a.dtype, np.integer) or a.size == 0):
        raise ValueError('seed_levels must be None, one sequence of int '
                         'levels shared by all streams, or [B, n]: the same '
                         'number of seed levels for every stream')
    if a.ndim == 1:
        a = np.broadcast_to(a, (B, a.shape[0]))
    if a.shape[0] != B:
        raise ValueError('seed_levels has %d rows for %d streams'
                         % (a.shape[0], B))
    if a.shape[1] < 1:
        raise ValueError('seed_levels needs at least one level per stream')
    if a.min() < 0 or a.max() > mol.TOP:
        raise ValueError('seed_levels must lie in 0 .. %d' % mol.TOP)
    return np.array(a, dtype=np.int32, order='C')   # (a writable copy)


def _mol_last(last, B):
    last = _batch_last(last, B)
    if not isinstance(last, torch.Tensor) and last.size and \
            (last.min() < 0 or last.max() > mol.TOP):
        raise ValueError('last_levels must lie in 0 .. %d' % mol.TOP)
    return last


def mol_batch_reset(net, g):
    _lib.call('wn_fastgen_mol_init', _lib.ptr(g['state']), g['state'].numel(),
              _lib.ptr(g['cursors']), _lib.ptr(g['hist']), g['B'],
              _lib.stream())
    g['steps'] = 0
    if g['restarted']:
        g['origin'].zero_()
        g['restarted'] = False


def generate_mixture_batch(net, num_samples, seeds, seed_levels, temperature,
                           global_condition, return_params_every, lc=None,
                           reserve_steps=None):
    _mol_need(net, 'generate_mixture_batch', 'generate_batch')
    reserve = _reserve_arg(reserve_steps)

    def per_stream(B):
        levels = _mol_levels(seed_levels, B)
        if not net.Lc and lc is None:
            return levels, None
        return levels, lcond.fastgen_rows(
            net, lc, 'generate_mixture_batch',
            levels.shape[1] + int(num_samples) - 1, B)
    sd, (levels, lc), gc, n = _batch_args(net, seeds, per_stream,
                                          global_condition, temperature,
                                          num_samples, mixture=True)
    B, n_given = levels.shape
    lc = _lc_device(net, lc)
    out = torch.zeros((B, n_given + n), dtype=torch.int32, device=net.device)
    out[:, :n_given] = torch.from_numpy(levels).to(net.device)
    g = batch_generator(net, B)
    mol_batch_reset(net, g)
    g['reserve'] = reserve

    def prime():
        # ONE forward pass per distinct (seed, GC id, LC rows), as
        # generate_batch; the history gets the seed's last 64 levels
        mol_batch_reset(net, g)
        n0, groups = n_given - 1, {}
        lch = None if lc is None else lc[:, :n0].cpu().numpy()
        for b in range(B):
            key = (levels[b, :n0].tobytes(),
                   None if gc is None else int(gc[b]),
                   None if lch is None else lch[b % len(lch)].tobytes())
            groups.setdefault(key, []).append(b)
        _prime(net, g, n0, [
            (torch.from_numpy(np.ascontiguousarray(levels[s[0], :n0])),
             None if gc is None else gc[s[0]:s[0] + 1], s,
             None if lc is None else lc[s[0] % lc.shape[0], :n0])
            for s in groups.values()], g['Bp'])
        g['cursors'][0] = n0
        t = np.arange(max(0, n0 - MOL_HIST), n0)
        hist = np.full((g['Bp'], MOL_HIST), -1, np.int32)
        hist[:B, t % MOL_HIST] = levels[:, t]
        g['hist'].copy_(torch.from_numpy(hist))
        g['steps'] = n0
    pe = int(return_params_every)
    params = _seeded(net, out, n_given, n, pe, prime, functools.partial(
        _batch_run, net, g, temperature, sd, gc), lc, (3, net.mol_K))
    return (out, params) if pe > 0 else out


def continue_mixture_batch(net, num_samples, last_levels, seeds, temperature,
                           global_condition, return_params_every, lc=None,
                           restart=None, reserve_steps=None):
    _mol_need(net, 'continue_mixture_batch', 'continue_generation_batch')
    reserve = _reserve_arg(reserve_steps)
    restart = _batch_restart_arg(restart, len(seeds))

    def per_stream(B):
        last = _mol_last(last_levels, B)
        if not net.Lc and lc is None:
            return last, None
        return last, lcond.fastgen_rows(net, lc, 'continue_mixture_batch',
                                        int(num_samples), B)
    sd, (last, lc), gc, n = _batch_args(net, seeds, per_stream,
                                        global_condition, temperature,
                                        num_samples, mixture=True)
    B = len(sd)
    g = net._bgen
    if g is None or g['B'] != B:
        raise RuntimeError('no batched generation of %d streams to '
                           'continue: call generate_mixture_batch first' % B)
    lc = _lc_device(net, lc)
    io = torch.zeros((B, n + 1), dtype=torch.int32, device=net.device)
    io[:, 0] = last if isinstance(last, torch.Tensor) else \
        torch.from_numpy(last).to(net.device)
    g['reserve'] = reserve
    if restart:
        flags = np.zeros(g['Bp'], np.int32)
        flags[restart] = 1
        g['flags'].copy_(torch.from_numpy(flags))
        _lib.call('wn_fastgen_mol_restart', _lib.ptr(g['state']),
                  _lib.ptr(g['dil']), net.L, B, _lib.ptr(g['cursors']),
                  _lib.ptr(g['hist']), _lib.ptr(g['origin']),
                  _lib.ptr(g['flags']), _lib.stream())
        g['restarted'] = True
    pe = int(return_params_every)
    params = _seeded(net, io, 1, n, pe, None, functools.partial(
        _batch_run, net, g, temperature, sd, gc), lc, (3, net.mol_K))
    return (io[:, 1:], params) if pe > 0 else io[:, 1:]
