"""Guard bands (tests/guard.py) around every operand of the entries of
include/wavenet_fastgen_mol.h that write through a pointer, at B = 5 streams
(Bp = 32 rows) and K = 10 components (Kp = 12): nothing outside the operands
is read or written.  Poison INSIDE operands where nothing may depend on it:
the padded columns k >= K of the pending logits, the history slots of the
rows >= B, and the LC ring's margins: its bands and every ring row that the
launch has no business reading (R = 4 rows; a step at T0 forms the
pre-activations of T0 + 1 and reads row (T0 + 1) % R only, wn_fastgen_mol_pre
row T0 % R only).  Each launch runs with two different poisons and must give
the same bits.
tests/test_fastgen_mol_host.py holds ENTRIES against the header."""
import numpy as np
import pytest
import torch

import guard

pytestmark = pytest.mark.gpu

# the entries of wavenet_fastgen_mol.h that write through a pointer
ENTRIES = ('wn_fastgen_mol_init', 'wn_fastgen_mol_pre', 'wn_fastgen_mol_step',
           'wn_fastgen_mol_finish', 'wn_fastgen_mol_restart')

B, BP, K, KP, K0, S = 5, 32, 10, 12, 32, 100
Q = 3 * KP
DIL = [1, 2, 4, 8, 16, 32] * 2
L = len(DIL)
ROWS = sum(DIL)
LSTRIDE = 5 * 1024 + 96            # a layer block without global conditioning
T0, BASE, LD, PROWS, R = 70, 68, 8, 8, 4
LSM = -14.0


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _f32bits(x):
    return int(np.float32(x).view(np.int32))


def _arena(poison, lc, origins, ring_row=None):
    """Every operand of a step at lock-step step T0 with a draw pending.
    poison: (float in the logits' padded columns and in the LC ring's rows
    other than ring_row, level in the history rows >= B)."""
    rng = np.random.default_rng(1)
    ar = guard.Arena('cuda')

    def f(name, shape, scale, role='in', **kw):
        return ar.place(name, (scale * rng.standard_normal(shape)).astype(
            np.float32), torch.float32, role=role, **kw)
    f('causal', (K0, 32), 0.3)
    f('layers', (L, LSTRIDE), 0.15)
    f('skip_w', (L * 32, S), 0.1)
    f('bsum', (S,), 0.1)
    f('post1_w', (S, S), 0.1)
    f('post1_b', (S,), 0.1)
    f('post2_w', (S, Q), 0.1)
    f('post2_b', (Q,), 0.1)
    f('bias', (L, 1, 64), 0.1)
    if lc:
        ring = (0.1 * rng.standard_normal((R, L, B, 64))).astype(np.float32)
        ring[[r for r in range(R) if r != ring_row]] = poison[0]
        ar.place('ring', ring, torch.float32)
    ar.place('dil', np.asarray(DIL, np.int32), torch.int32, fill=(1, 2))
    f('state', (ROWS, BP, 32), 0.5, role='inout')
    ar.place('cursors', np.asarray([T0, 1, 0, 0], np.int32), torch.int32,
             role='inout')
    hist = rng.integers(0, 65536, (BP, 64)).astype(np.int32)
    hist[0, :4] = [0, 1, 65534, 65535]
    hist[B:] = poison[1]
    ar.place('hist', hist, torch.int32, role='inout', fill=(0, 65535))
    io = rng.integers(0, 65536, (B, LD)).astype(np.int32)
    ar.place('io', io, torch.int32, role='inout', fill=(0, 65535))
    ctl = np.asarray([BASE, 1, 1, _f32bits(0.7), LD, PROWS, 0, 0], np.int32)
    ar.place('ctl', ctl, torch.int32)
    ar.place('seeds', np.arange(11, 11 + B, dtype=np.int64), torch.int64)
    ar.place('params', (B, PROWS, 3, K), torch.float32, role='out')
    f('pre', (L, BP, 64), 0.3, role='inout')
    ar.place('z_all', (BP, L * 32), torch.float32, role='out')
    ar.place('h1', (BP, S), torch.float32, role='out')
    ar.place('h2', (BP, S), torch.float32, role='out')
    lg = (0.5 * rng.standard_normal((BP, Q))).astype(np.float32)
    for blk in range(3):
        lg[:, blk * KP + K:(blk + 1) * KP] = poison[0]
    ar.place('logits', lg, torch.float32, role='inout')
    if origins:
        ar.place('origin', np.asarray([0, 3, 0, 60, 0] + [0] * (BP - B),
                                      np.int32), torch.int32, role='inout',
                 fill=(0, 1))
    return ar


POISONS = ((float('nan'), 777), (1e30, 40000))


def _both(build, run, outs):
    """The launch under both poisons: bands intact, outputs independent of
    the bands and of the poison."""
    seen = []
    for poison in POISONS:
        ar = build(poison)
        bits = guard.read_check(ar, lambda: run(ar))
        ar.check()
        seen.append({k: bits[k].clone() for k in outs})
    for k in outs:
        assert torch.equal(seen[0][k], seen[1][k]), k
    return seen[0]


@pytest.mark.parametrize('lc,origins', [(False, False), (True, True)])
def test_step_stays_inside_its_operands(hip_lib, lc, origins):
    def run(ar):
        p = ar.ptr
        assert hip_lib.wn_fastgen_mol_step(
            p('causal'), K0, p('layers'), LSTRIDE, p('skip_w'), p('bsum'),
            p('post1_w'), p('post1_b'), p('post2_w'), p('post2_b'),
            p('bias'), 0, p('dil'), L, S, K, B, p('state'), p('cursors'),
            p('hist'), p('io'), p('ctl'), p('seeds'), p('params'), 1, LSM,
            p('pre'), p('z_all'), p('h1'), p('h2'), p('logits'),
            p('ring') if lc else None, R if lc else 0, 64 if lc else 0,
            p('origin') if origins else None, _stream()) == 0
    outs = ['state', 'cursors', 'io', 'params', 'pre', 'z_all', 'h1', 'h2',
            'logits']
    bits = _both(lambda po: _arena(po, lc, origins, (T0 + 1) % R), run, outs)
    assert bits['cursors'].tolist()[:2] == [T0 + 1, 1]
    for k in ('z_all', 'h1', 'h2', 'logits', 'pre'):
        got = bits[k].cpu().numpy().view(np.float32)
        assert np.isfinite(got).all(), k
    row = bits['params'].cpu().numpy().view(np.float32)[:, 1]
    assert np.isfinite(row).all()
    lv = bits['io'].cpu().numpy()[:, 2]
    assert (lv >= 0).all() and (lv <= 65535).all()


def test_step_history_gets_the_level_and_nothing_else(hip_lib):
    ar = _arena(POISONS[1], False, False)
    before = ar['hist'].clone()
    p = ar.ptr
    assert hip_lib.wn_fastgen_mol_step(
        p('causal'), K0, p('layers'), LSTRIDE, p('skip_w'), p('bsum'),
        p('post1_w'), p('post1_b'), p('post2_w'), p('post2_b'), p('bias'), 0,
        p('dil'), L, S, K, B, p('state'), p('cursors'), p('hist'), p('io'),
        p('ctl'), p('seeds'), p('params'), 1, LSM, p('pre'), p('z_all'),
        p('h1'), p('h2'), p('logits'), None, 0, 0, None, _stream()) == 0
    torch.cuda.synchronize()
    ar.check()
    after = ar['hist']
    slot = T0 & 63
    assert torch.equal(after[:B, slot], ar['io'][:, T0 - BASE])
    keep = torch.ones(64, dtype=torch.bool)
    keep[slot] = False
    keep = keep.to(after.device)
    assert torch.equal(after[:, keep], before[:, keep])
    assert torch.equal(after[B:], before[B:])


def test_finish_stays_inside_its_operands(hip_lib):
    def run(ar):
        p = ar.ptr
        assert hip_lib.wn_fastgen_mol_finish(
            K, LSM, B, p('cursors'), p('io'), p('ctl'), p('seeds'),
            p('params'), p('logits'), None, _stream()) == 0
    bits = _both(lambda po: _arena(po, False, False), run,
                 ['cursors', 'io', 'params'])
    assert bits['cursors'].tolist()[:2] == [T0, 0]
    assert np.isfinite(bits['params'].cpu().numpy().view(np.float32)[:, 1]).all()


def test_pre_stays_inside_its_operands(hip_lib):
    for lc in (False, True):
        def run(ar):
            p = ar.ptr
            assert hip_lib.wn_fastgen_mol_pre(
                p('layers'), LSTRIDE, p('bias'), 0, p('dil'), L, B,
                p('state'), p('cursors'), p('pre'),
                p('ring') if lc else None, R if lc else 0, 64 if lc else 0,
                _stream()) == 0
        bits = _both(lambda po: _arena(po, lc, False, T0 % R), run, ['pre'])
        got = bits['pre'].cpu().numpy().view(np.float32).reshape(L, BP, 64)
        assert np.isfinite(got).all() and not got[:, B:].any()


def test_init_stays_inside_its_operands(hip_lib):
    ar = guard.Arena('cuda')
    ar.place('state', (ROWS, BP, 32), torch.float32, role='out')
    ar.place('cursors', (4,), torch.int32, role='out')
    ar.place('hist', (BP, 64), torch.int32, role='out', fill=(7, 9))

    def run():
        assert hip_lib.wn_fastgen_mol_init(
            ar.ptr('state'), ROWS * BP * 32, ar.ptr('cursors'),
            ar.ptr('hist'), B, _stream()) == 0
    bits = guard.read_check(ar, run)
    ar.check()
    assert not bits['state'].any() and not bits['cursors'].any()
    assert (bits['hist'] == -1).all()


def test_restart_stays_inside_its_operands(hip_lib):
    flags = np.zeros(BP, np.int32)
    flags[[1, 4]] = 1
    flags[B:] = 1                  # (rows past B are never streams)

    def build(poison):
        ar = _arena(poison, False, True)
        ar.place('flags', flags, torch.int32, fill=(0, 1))
        return ar

    def run(ar):
        p = ar.ptr
        assert hip_lib.wn_fastgen_mol_restart(
            p('state'), p('dil'), L, B, p('cursors'), p('hist'), p('origin'),
            p('flags'), _stream()) == 0
    bits = _both(build, run, ['state', 'cursors', 'origin'])
    ar = build(POISONS[0])
    before = {k: ar[k].clone() for k in ('state', 'hist', 'origin')}
    run(ar)
    torch.cuda.synchronize()
    ar.check()
    on = torch.zeros(BP, dtype=torch.bool)
    on[[1, 4]] = True
    on = on.to(ar['hist'].device)
    assert (ar['hist'][on] == -1).all()
    assert torch.equal(ar['hist'][~on], before['hist'][~on])
    assert not ar['state'][:, on].any()
    assert torch.equal(ar['state'][:, ~on].view(torch.int32),
                       before['state'][:, ~on].view(torch.int32))
    assert ar['origin'][on].tolist() == [T0, T0]
    assert torch.equal(ar['origin'][~on], before['origin'][~on])
    assert bits['cursors'].tolist()[:2] == [T0, 1]
