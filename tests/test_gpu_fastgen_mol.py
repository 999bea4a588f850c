"""Batched fast generation for mixture-of-logistics models on the device
(WaveNetModel.generate_mixture_batch, csrc/wn_fastgen_mol.hip): teacher-forced
parameters against the float64 network of tests/mol_ref.py, every draw of a
free run against mol.sample_reference, batch invariance, chunking, priming,
restarts (all bit for bit) and generate.py --fast_mixture.

Worst teacher-forced error seen on an MI355X, as a share of the bound 2e-5 x
max(1, largest |float64 head output|): see the README's section on this
path; the test prints it for every case."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import lc_ref
import mol_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIL = [1, 2, 4, 8, 16, 32] * 2
S, GC, CARD, LC = 100, 8, 10, 5
TOL = 2e-5      # of max(1, largest |float64 head output|): the project's bar
EDGE = [0, 1, 65534, 65535]


def _model(K, K0, plain=False, lc=False, seed=0):
    from wavenet import WaveNetModel
    kw = {}
    if not plain:
        kw.update(global_condition_channels=GC,
                  global_condition_cardinality=CARD)
    if lc:
        kw['local_condition_channels'] = LC
    net = WaveNetModel(1, DIL, 2, 32, 32, S, quantization_channels=64,
                       use_biases=not plain, scalar_input=True,
                       initial_filter_width=K0, output_mixture=K, seed=seed,
                       **kw)
    g = torch.Generator().manual_seed(seed + 11)
    with torch.no_grad():
        for n, v in net.named_variables():
            last = n.split('/')[-1]
            if 'bias' in last:
                v.copy_((0.1 * torch.randn(v.shape, generator=g,
                                           dtype=torch.float64)).float())
            elif last.startswith('lc_'):
                v.copy_((0.3 * torch.randn(v.shape, generator=g,
                                           dtype=torch.float64)).float())
        if not plain:
            # scales round e^-2 of full scale (tests/test_gpu_mol_model.py)
            Kp = net.mol_Kp
            net.variables['postprocessing']['postprocess2_bias'][
                2 * Kp:2 * Kp + K] -= 2.0
    net.fastgen_graph_steps = 40       # captured and single steps both run
    return net


def _levels(B, n, seed):
    lv = np.random.default_rng(seed).integers(0, 65536, (B, n)).astype(np.int32)
    k = min(n, 4)
    lv[0, :k] = EDGE[:k]
    lv[-1, n - k:] = EDGE[4 - k:]
    return lv


def _float64_params(net, levels, ids, lc=None):
    """[B, n, 3, K] float64 and the largest |head output| of the float64
    network on the levels' centres."""
    from wavenet import mol
    x = torch.as_tensor(mol.centres(levels).astype(np.float64))
    v = lc_ref._to_torch(lc_ref.model_tree(net))
    with torch.no_grad():
        raw = R.forward(v, DIL, x, None if lc is None else torch.as_tensor(
            np.asarray(lc, np.float64)), ids, net.use_biases).numpy()
    K = net.mol_K
    out = np.stack([np.stack([R.params(raw[b, t], K, net.mol_log_scale_min)
                              for t in range(raw.shape[1])])
                    for b in range(raw.shape[0])])
    Kp = net.mol_Kp
    cols = np.concatenate([np.arange(blk * Kp, blk * Kp + K)
                           for blk in range(3)])
    return out, float(np.abs(raw[:, :, cols]).max())


def _worst(got, want, scale):
    bound = TOL * max(1.0, scale)
    return max(float(np.abs(got[:, :, blk] - want[:, :, blk]).max())
               for blk in range(3)) / bound


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


# ------------------------------------------------ teacher-forced parameters
CASES = [('k10_k0_32', 10, 32, False, False), ('k1_k0_2', 1, 2, False, False),
         ('k32_k0_3', 32, 3, False, False), ('k4_k0_1', 4, 1, False, False),
         ('k10_plain', 10, 32, True, False), ('k10_lc', 10, 4, False, True)]


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_teacher_forced_parameters_match_float64(hip_lib, case):
    name, K, K0, plain, lc = case
    B, n = 5, 150
    net = _model(K, K0, plain, lc, seed=len(name))
    levels = _levels(B, n, K)
    ids = None if plain else [3, 0, 9, 3, 7]
    rows = None
    if lc:
        rows = np.random.default_rng(2).standard_normal(
            (B, n, LC)).astype(np.float32)
    out, params = net.generate_mixture_batch(
        1, [5, 6, 7, 8, 2 ** 63 + 9], levels, 0.7, ids, 1,
        local_condition=rows)
    assert out.shape == (B, n + 1) and params.shape == (B, n, 3, K)
    assert torch.equal(out[:, :n].cpu(), torch.from_numpy(levels))
    want, scale = _float64_params(net, levels, ids, rows)
    ratio = _worst(params.cpu().numpy().astype(np.float64), want, scale)
    print('%s: worst error / bound %.3f (largest head output %.2f)'
          % (name, ratio, scale))
    assert ratio <= 1.0


# ------------------------------------------------------------- every draw
@pytest.mark.parametrize('tau', [0.7, 0.0])
def test_every_draw_is_the_reference_draw(hip_lib, tau):
    from wavenet import mol
    B, n, K = 5, 300, 10
    net = _model(K, 32, seed=4)
    seeds = [11, 12, 13, 2 ** 64 - 1, 0]
    first = np.asarray([[0], [65535], [32768], [1], [40000]], np.int32)
    out, params = net.generate_mixture_batch(n, seeds, first, tau,
                                             [1, 2, 3, 4, 5], 1)
    out, params = out.cpu().numpy(), params.cpu().numpy()
    assert out.shape == (B, n + 1) and params.shape == (B, n, 3, K)
    excused = wrong = 0
    for b in range(B):
        ctr = np.arange(n)
        lv, _, x = mol.sample_reference(params[b], [seeds[b]] * n, ctr, tau,
                                        return_x=True)
        for t in np.nonzero(lv != out[b, 1:])[0]:
            frac = (np.clip(x[t], -1, 1) + 1) * 32767.5
            near_round = abs(frac - np.floor(frac) - 0.5) < 1e-6
            pk = np.exp(params[b, t, 0].astype(np.float64))
            u1 = mol.draw_uniform(seeds[b], 2 * int(t))
            near_pick = np.abs(np.cumsum(pk) / pk.sum() - u1).min() < 1e-12
            if near_round or near_pick:
                excused += 1
            else:
                wrong += 1
    print('tau %.1f: %d of %d draws excused at a boundary' % (tau, excused,
                                                             B * n))
    assert wrong == 0 and excused <= B * n // 100
    assert len(np.unique(out[:, 1:])) > 50
    assert out.min() >= 0 and out.max() <= 65535


# ------------------------------------------------------- batch invariance
def test_streams_do_not_depend_on_the_batch(hip_lib):
    B, n, K = 37, 70, 10
    net = _model(K, 32, seed=5)
    seeds = [100 + b for b in range(B)]
    first = _levels(B, 3, 8)
    ids = [b % CARD for b in range(B)]
    out, params = net.generate_mixture_batch(n, seeds, first, 0.9, ids, 1)
    for b in (0, 31, 32, 36):
        o1, p1 = net.generate_mixture_batch(n, [seeds[b]], first[b:b + 1],
                                            0.9, [ids[b]], 1)
        assert torch.equal(o1[0], out[b]), b
        assert torch.equal(_bits(p1[0]), _bits(params[b])), b
        # the single-stream call is that call, squeezed
        o2, p2 = net.generate_mixture(n, first[b], 0.9, [ids[b]], seeds[b], 1)
        assert torch.equal(o2, out[b]) and torch.equal(_bits(p2), _bits(p1[0]))


# --------------------------------------------------------------- chunking
def test_two_calls_are_one(hip_lib):
    B, K = 3, 4
    net = _model(K, 32, seed=6)
    seeds, ids = [1, 2, 3], [0, 4, 9]
    first = _levels(B, 2, 3)
    whole, pw = net.generate_mixture_batch(130, seeds, first, 0.8, ids, 1)
    a, pa = net.generate_mixture_batch(70, seeds, first, 0.8, ids, 1)
    b, pb = net.continue_mixture_batch(60, a[:, -1], seeds, 0.8, ids, 1)
    assert torch.equal(torch.cat([a, b], 1), whole)
    assert torch.equal(_bits(torch.cat([pa, pb], 1)), _bits(pw))
    # one stream, through the squeezed calls
    a1 = net.generate_mixture(70, first[1], 0.8, [ids[1]], seeds[1])
    b1 = net.continue_mixture(60, int(a1[-1]), 0.8, [ids[1]], seeds[1])
    assert torch.equal(torch.cat([a1, b1]), whole[1])


# ---------------------------------------------------------------- priming
def test_priming_by_the_forward_pass(hip_lib):
    B, K, n0, n1, n2 = 3, 10, 100, 5, 12
    net = _model(K, 32, seed=7)
    net.fastgen_prime_forward_min = 50
    seeds, ids = [21, 22, 23], [1, 1, 6]
    seed_lv = _levels(B, n0, 9)
    seed_lv[1] = seed_lv[0]            # two streams share one forward pass
    a = net.generate_mixture_batch(n1, seeds, seed_lv, 0.8, ids)
    b, pb = net.continue_mixture_batch(n2, a[:, -1], seeds, 0.8, ids, 1)
    full = torch.cat([a, b], 1).cpu().numpy()
    assert full.shape == (B, n0 + n1 + n2)
    # the same levels stepped through one by one (a parameter row asked
    # for: no forward pass), and the float64 network
    net.fastgen_prime_forward_min = 10 ** 9
    _, ps = net.generate_mixture_batch(1, seeds, full[:, :-1], 0.8, ids, 1)
    want, scale = _float64_params(net, full[:, :-1], ids)
    lo = n0 + n1 - 1                   # the step that consumed a[:, -1]
    got = pb.cpu().numpy().astype(np.float64)
    r_primed = _worst(got, want[:, lo:lo + n2], scale)
    r_step = _worst(ps.cpu().numpy().astype(np.float64), want, scale)
    print('primed: worst error / bound %.3f; stepped %.3f' % (r_primed,
                                                              r_step))
    assert r_primed <= 1.0 and r_step <= 1.0
    # primed streams are batch invariant, bit for bit
    net.fastgen_prime_forward_min = 50
    for s in (0, 2):
        a1 = net.generate_mixture_batch(n1, [seeds[s]], seed_lv[s:s + 1], 0.8,
                                        [ids[s]])
        b1, p1 = net.continue_mixture_batch(n2, a1[:, -1], [seeds[s]], 0.8,
                                            [ids[s]], 1)
        assert torch.equal(a1[0], a[s]) and torch.equal(b1[0], b[s])
        assert torch.equal(_bits(p1[0]), _bits(pb[s]))


# ---------------------------------------------------------------- restart
def test_a_restarted_stream_is_a_fresh_one(hip_lib):
    B, K = 3, 10
    net = _model(K, 32, seed=8)
    seeds, ids = [31, 32, 33], [2, 5, 8]
    first = _levels(B, 1, 4)
    a = net.generate_mixture_batch(90, seeds, first, 0.8, ids)
    b, pb = net.continue_mixture_batch(45, a[:, -1], seeds, 0.8, ids, 1,
                                       restart=[2])
    c, pc = net.continue_mixture_batch(30, b[:, -1], seeds, 0.8, ids, 1)
    last = int(a[2, -1])
    fresh, pf = net.generate_mixture_batch(75, [seeds[2]], [[last]], 0.8,
                                           [ids[2]], 1)
    assert torch.equal(torch.cat([b[2], c[2]]), fresh[0, 1:])
    assert torch.equal(_bits(torch.cat([pb[2], pc[2]])), _bits(pf[0]))
    # the other streams went on as if nothing had happened
    whole = net.generate_mixture_batch(165, seeds, first, 0.8, ids)
    assert torch.equal(torch.cat([a, b, c], 1)[:2], whole[:2])


# ----------------------------------------------------------- command line
PARAMS = {"filter_width": 2, "sample_rate": 16000, "dilations": [1, 2, 4],
          "residual_channels": 32, "dilation_channels": 32,
          "quantization_channels": 64, "skip_channels": 32,
          "use_biases": True, "scalar_input": True,
          "initial_filter_width": 4, "residual_postproc": False}


def _child(script, argv, seconds=300):
    p = subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv,
                       cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=seconds)
    return p.returncode, p.stdout.decode()


def _npy(logdir):
    found = []
    for d, _, files in os.walk(logdir):
        found += [os.path.join(d, f) for f in files
                  if f == 'generated_levels.npy']
    assert len(found) == 1, found
    return np.load(found[0])


def test_generate_fast_mixture(hip_lib, tmp_path):
    import train
    from wavenet import mol
    from wavenet.cli import model_from_params
    params = str(tmp_path / 'params.json')
    json.dump(PARAMS, open(params, 'w'))
    code, out = _child('train.py', [
        '--synthetic', '--wavenet_params', params, '--sample_size', '1000',
        '--batch_size', '1', '--num_steps', '1', '--checkpoint_every', '10',
        '--logdir', str(tmp_path / 'run'), '--output_mixture', '4'])
    assert code == 0, out
    ck_path = train.latest_checkpoint(str(tmp_path / 'run'))
    n, seed, tau = 60, 3, 0.8
    common = [ck_path, '--wavenet_params', params, '--samples', str(n),
              '--seed', str(seed), '--temperature', str(tau),
              '--fast_mixture', 'true']
    ck = torch.load(ck_path, map_location='cpu')
    net = model_from_params(PARAMS, 1, **mol.model_keywords(
        mol.check_entry(ck['output'])))
    net.load_state_dict(ck['variables'])
    lv0 = np.random.default_rng(seed).integers(65536, size=(1,))
    # one stream, in two chunks
    wav = str(tmp_path / 'one.wav')
    code, out = _child('generate.py', common + [
        '--wav_out_path', wav, '--logdir', str(tmp_path / 'log1'),
        '--save_every', '25'])
    assert code == 0, out
    want = net.generate_mixture(n, lv0, tau, seed=seed).cpu().numpy()
    got = _npy(str(tmp_path / 'log1'))
    assert got.dtype == np.int32 and got.tolist() == want[1:].tolist()
    rate, pcm = wavfile.read(wav)
    assert rate == 16000 and pcm.dtype == np.int16
    assert pcm.astype(np.int32).tolist() == (want - 32768).tolist()
    assert len(set(want.tolist())) > 3
    # three clips
    wav = str(tmp_path / 'clips.wav')
    code, out = _child('generate.py', common + [
        '--wav_out_path', wav, '--logdir', str(tmp_path / 'log3'),
        '--clips', '3'])
    assert code == 0, out
    want = net.generate_mixture_batch(
        n, [seed, seed + 1, seed + 2], lv0, tau).cpu().numpy()
    got = _npy(str(tmp_path / 'log3'))
    assert got.shape == (3, n) and np.array_equal(got, want[:, 1:])
    for i in range(3):
        _, pcm = wavfile.read(str(tmp_path / ('clips_%d.wav' % i)))
        assert pcm.astype(np.int32).tolist() == (want[i] - 32768).tolist()
    assert not np.array_equal(want[0], want[1])
    # a softmax checkpoint: the flag is an error that names itself
    code, out = _child('train.py', [
        '--synthetic', '--wavenet_params', params, '--sample_size', '1000',
        '--batch_size', '1', '--num_steps', '1', '--checkpoint_every', '10',
        '--logdir', str(tmp_path / 'soft')])
    assert code == 0, out
    code, out = _child('generate.py', [
        train.latest_checkpoint(str(tmp_path / 'soft')), '--wavenet_params',
        params, '--samples', '4', '--fast_mixture', 'true'])
    assert code == 1 and '--fast_mixture' in out and 'softmax' in out, out
