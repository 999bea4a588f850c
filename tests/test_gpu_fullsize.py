"""BASELINE.json-sized runs (default stack, B=8, T=16000) checked through
size-independent properties of the domain: clip independence (DP identity),
causality, loss-mean decomposition, determinism -- plus the behavioural
training thresholds of the reference's test/test_model.py."""
import json
import os

import numpy as np
import pytest
import torch

from util import O, ROOT, DEFAULT, cfg_with, model_kwargs, synth_audio

pytestmark = pytest.mark.gpu


def default_cfg(B):
    p = json.load(open(os.path.join(ROOT, 'wavenet_params.json')))
    c = {k: p[k] for k in p if k != 'sample_rate'}
    c['batch_size'] = B
    return c


GOLD = os.path.join(ROOT, 'tests', 'golden')
GRAD_REL = 2e-5


def _var_tols(names, tag='config1'):
    """Per variable: max(2e-5, 4 x the float32 ORACLE's own error on that
    configuration at full length) -- tests/golden/config{1,4}_fullsize.npz,
    generated in the build container by tests/golden/make_golden.py
    (fp32_error)."""
    fx = np.load(os.path.join(GOLD, tag + '_fullsize.npz'))
    e32 = dict(zip([str(n) for n in fx[tag + '/names']], fx[tag + '/err32']))
    return np.array([max(GRAD_REL, 4.0 * float(e32[n])) for n in names])


def _flat_grads(net):
    from util import flat_named, tree_to_numpy
    return flat_named(tree_to_numpy(net.gradients))


def _log(tag, payload, name='fullsize_errors.json'):
    out = os.path.join(ROOT, 'gpurun_out')
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, name)
    try:
        cur = json.load(open(path))
    except (OSError, ValueError):
        cur = {}
    cur[tag] = payload
    json.dump(cur, open(path, 'w'), indent=1)


@pytest.mark.parametrize('gc', [False, True], ids=['config2', 'config4_gc'])
def test_full_size_dp_identity_and_determinism(hip_lib, monkeypatch, gc):
    """grad(B=8) == mean of the eight single-clip gradients, loss
    likewise -- EVERY variable within max(2e-5, 4 x the float32 oracle's own
    error) of that variable's largest entry; two runs are bitwise identical
    (slab reductions, no float atomics).  Clip 0 of the batch is the clip
    test_config1_full_length_vs_oracle pins against the float64 oracle.
    Both sides on 32-row tiles: a single clip would by default run the 16-row
    stack launches, whose activations differ from the 32-row ones in the last
    bits -- enough to put a handful of the 16000 x 512 post-processing ReLUs on
    the other side of their kink (test_config1_full_length_vs_oracle counts 7
    against 11 such positions for the two tile heights), and a gradient is not
    continuous there: the two heights agree with the float64 oracle to 3e-6 of
    a variable EACH, taking their own side at those kinks, and with each other
    only to 1.7e-3.  The identity under test is the sharding's.
    gc: BASELINE.json configs[3]'s per-GPU batch -- global conditioning 32 x 377
    with eight DISTINCT speaker ids (37 b mod 377): the embedding rows and the
    gc_filtweights / gc_gateweights gradients (model.py:272-284, 533-562) under
    the same per-variable rule."""
    from wavenet import WaveNetModel
    from wavenet._lib import stack_variant
    monkeypatch.setattr(WaveNetModel, 'DEFAULT_STACK_VARIANT', stack_variant(rows=32))
    T = 16000
    audio = synth_audio(8, T)
    extra = dict(global_condition_channels=32, global_condition_cardinality=377) if gc else {}
    ids = np.array([(37 * b) % 377 for b in range(8)], np.int32) if gc else None
    net8 = WaveNetModel(seed=0, **model_kwargs(dict(default_cfg(8), **extra)))
    l8 = float(net8.loss(audio, ids))
    g8 = net8.grads.clone()
    l8b = float(net8.loss(audio, ids))
    assert l8 == l8b and torch.equal(g8, net8.grads)
    named8 = _flat_grads(net8)
    net1 = WaveNetModel(seed=0, **model_kwargs(dict(default_cfg(1), **extra)))
    assert torch.equal(net1.params, net8.params)
    lsum, acc = 0.0, None
    for b in range(8):
        lsum += float(net1.loss(audio[b:b + 1], None if ids is None else ids[b:b + 1]))
        g = [a.astype(np.float64) for _, a in _flat_grads(net1)]
        acc = g if acc is None else [x + y for x, y in zip(acc, g)]
    assert abs(lsum / 8 - l8) < 1e-5
    names = [n for n, _ in named8]
    tols = _var_tols(names, 'config4' if gc else 'config1')
    worst, bad = (0.0, ''), []
    for (n, a), m, tol in zip(named8, acc, tols):
        m = m / 8
        sc = np.abs(m).max()
        err = np.abs(a - m).max()
        if sc > 0:
            worst = max(worst, (err / sc, n))
        if not err <= tol * sc + 1e-12:
            bad.append((n, float(err), float(sc), float(tol)))
    _log('dp_identity_B8_vs_8xB1' + ('_gc' if gc else ''), {'worst_ratio': worst, 'bad': bad[:10]})
    if gc:
        # every one of the eight speakers' embedding rows got a gradient
        emb = dict(named8)['wavenet/embeddings/gc_embedding']
        assert all(np.abs(emb[i]).max() > 0 for i in ids) and \
            np.count_nonzero(np.abs(emb).max(axis=1)) == 8
    assert not bad, bad[:6]


_ORACLE64 = {}


def _oracle64(tag, cfg, var, audio, ids, fx):
    """float64 oracle of a full-length fixture, run ONCE per test session and
    checked against the committed fingerprints (step 1 of
    test_full_length_vs_oracle): (loss, forward cache incl. every logits row)."""
    if tag in _ORACLE64:
        return _ORACLE64[tag]
    from make_golden import sample_index
    from util import flat_named
    l64, g64 = O.loss_and_grads(cfg, var, audio, ids, dtype=np.float64)
    assert abs(l64 - float(fx[tag + '/loss'])) < 1e-12
    flat64 = flat_named(g64)
    assert [n for n, _ in flat64] == [str(n) for n in fx[tag + '/names']]
    for i, (n, a) in enumerate(flat64):
        sc = float(fx[tag + '/absmax'][i])
        assert abs(np.abs(a).max() - sc) <= 1e-9 * sc + 1e-300, n
        assert abs(a.sum() - fx[tag + '/sum'][i]) <= 1e-9 * fx[tag + '/abssum'][i] + 1e-300, n
        assert abs(np.abs(a).sum() - fx[tag + '/abssum'][i]) <= 1e-9 * fx[tag + '/abssum'][i] + 1e-300, n
        got = a.reshape(-1)[sample_index(a.size, i)]
        assert np.abs(got - fx[tag + '/samples'][i]).max() <= 2e-7 * sc + 1e-300, n
    _, c = O.loss(cfg, var, audio, ids, None, np.float64, keep=True)
    _ORACLE64[tag] = (l64, c)
    return _ORACLE64[tag]


def _compare_with_oracle(hip_lib, net, cfg, var, audio, ids, l64, c, tols_tag, rows,
                         max_flips=None):
    """Steps 2 - 4 of test_full_length_vs_oracle for one model / kernel path;
    returns the log entry."""
    from util import flat_named, oracle_grads_at_device_kinks
    B, T = audio.shape
    # (the backward pass turns the logits into their gradient in place)
    loss_fwd = float(net.loss(audio, ids, backward=False))
    ws = [w for w in net._ws.values() if w.T == T][0]
    lg = ws.logits.cpu().numpy().reshape(B, T, -1)
    loss = float(net.loss(audio, ids))
    torch.cuda.synchronize()
    assert loss == loss_fwd
    wst = [w for w in net._ws.values() if w.T == T and w.training][0]
    # the launches under test are the ones that ran
    assert wst.stack_rows == rows == hip_lib.wn_stack_tile_rows(B, T, wst.stack_variant)
    assert net.stack_fwd and wst.stack_bwd and net._stack_bwd_ok()
    # (2) loss; EVERY logits row
    assert abs(loss - l64) < 1e-5
    logits_err = float(np.abs(lg - c['logits']).max())
    assert logits_err < 1e-4, logits_err
    # (3) + (4)
    ref_loss, ref_g, _, flips = oracle_grads_at_device_kinks(net, cfg, var, audio, ids,
                                                             cache=c)
    if max_flips is not None:
        assert flips <= max_flips
    named = _flat_grads(net)
    tols = _var_tols([n for n, _ in named], tols_tag)
    worst, bad = (0.0, ''), []
    for (n, a), (_, b), tol in zip(named, flat_named(ref_g), tols):
        sc = np.abs(b).max()
        err = np.abs(a - b).max()
        if sc > 0:
            worst = max(worst, (err / sc, n))
        if not err <= tol * sc + 1e-12:
            bad.append((n, float(err), float(sc), float(tol)))
    entry = {'tile_rows': rows, 'worst_ratio': worst, 'relu_flips': flips,
             'loss_err': abs(loss - l64), 'logits_rows_compared': B * T,
             'logits_max_err': logits_err, 'bad': bad[:10]}
    return entry, bad


@pytest.mark.parametrize('rows', [16, 32], ids=['rows16', 'rows32'])
@pytest.mark.parametrize('tag', ['config1', 'config4'])
def test_full_length_vs_oracle(hip_lib, tag, rows):
    """BASELINE.json configs[0] at FULL length (default stack, one clip of
    16000 samples) and one GPU's share of configs[3] (the same with global
    conditioning 32 x 377, global clip 5, speaker id 185): the committed
    float64 fingerprints (tests/golden/config{1,4}_fullsize.npz) pin the
    oracle, the oracle pins the device -- on BOTH tile heights of the stack
    launches: rows16 = what the library picks for one clip (stack_fwd16_kernel
    with the fused skip sum, stack_bwd16_kernel), rows32 = the launches of the
    benchmark's 8 x 16000 batch forced by the variant word
    (stack_fwd_kernel<2,16> + the K = 1600 skip GEMM + stack_bwd_kernel<8>).
      1. the float64 oracle run here reproduces the committed loss and every
         variable's sum / abs-sum / max / 32 sampled gradient entries;
      2. the device's loss equals it to 1e-5, ALL 16000 logits rows to 1e-4;
      3. the device's ReLU decisions differ from the oracle's only where the
         oracle's pre-activation is within 2e-5 of 0, at no more positions
         than the fixture counts there;
      4. every entry of every variable's gradient (config4: incl. the
         embedding table and every layer's gc_filtweights / gc_gateweights) is
         within max(2e-5, 4 x the float32 oracle's own error) of the
         variable's largest entry, against the float64 oracle taking the
         device's side at those kinks."""
    sys_path_golden()
    from make_golden import fullsize_inputs
    from util import build_pair
    from wavenet._lib import stack_variant
    fx = np.load(os.path.join(GOLD, tag + '_fullsize.npz'))
    cfg, audio, ids = fullsize_inputs(tag)
    assert np.allclose([audio.sum(dtype=np.float64), np.abs(audio).sum(dtype=np.float64)],
                       fx[tag + '/audio_crc'], rtol=0, atol=1e-9)
    net, var = build_pair(cfg)
    if rows == 32:
        net.stack_variant = stack_variant(rows=32)
    else:
        assert hip_lib.wn_stack_tile_rows(1, 16000, 0) == 16     # the library's own choice
    l64, c = _oracle64(tag, cfg, var, audio, ids, fx)
    # the committed first / last logits rows pin the live oracle's logits
    assert np.abs(c['logits'][0, 0] - fx[tag + '/logits_first_last'][0]).max() < 1e-9
    assert np.abs(c['logits'][0, -1] - fx[tag + '/logits_first_last'][1]).max() < 1e-9
    entry, bad = _compare_with_oracle(hip_lib, net, cfg, var, audio, ids, l64, c, tag, rows,
                                      max_flips=int(fx[tag + '/near_kink'].sum()))
    _log('%s_T16000_vs_float64%s' % (tag, '' if rows == 16 else '_rows32'), entry)
    assert not bad, bad[:6]


def test_natural_32_row_batch_vs_oracle(hip_lib):
    """B = 3, T = 11000 of the default stack: 1032 32-row tiles, one more than
    four per CU allows, so the LIBRARY picks the 32-row launches
    (stack_fwd_kernel<2,16>, stack_bwd_kernel<8>: the benchmark's kernels)
    without a forced variant -- loss, every logits row, every gradient entry
    against the float64 oracle, as in test_full_length_vs_oracle."""
    from util import build_pair
    cfg = default_cfg(3)
    B, T = 3, 11000
    assert hip_lib.wn_stack_tile_rows(B, T, 0) == 32
    audio = synth_audio(B, T, seed=77)
    net, var = build_pair(cfg)
    l64, c = O.loss(cfg, var, audio, None, None, np.float64, keep=True)
    entry, bad = _compare_with_oracle(hip_lib, net, cfg, var, audio, None, l64, c,
                                      'config1', 32)
    _log('default_B3_T11000_vs_float64_rows32_natural', entry)
    assert not bad, bad[:6]


def sys_path_golden():
    import sys
    if GOLD not in sys.path:
        sys.path.insert(0, GOLD)


def test_full_size_causality(hip_lib):
    """Changing samples at t >= t0 must not change logits before t0."""
    from wavenet import WaveNetModel
    T, t0 = 16000, 9000
    audio = synth_audio(1, T)
    net = WaveNetModel(seed=0, **model_kwargs(default_cfg(1)))
    net.loss(audio, backward=False)
    ws = list(net._ws.values())[0]
    a = ws.logits.clone()
    audio2 = audio.copy()
    audio2[0, t0:] = -audio2[0, t0:]
    net.loss(audio2, backward=False)
    b = ws.logits
    assert torch.equal(a[:t0], b[:t0])
    assert not torch.equal(a[t0:], b[t0:])


def test_default_stack_prefix_vs_oracle(hip_lib):
    """The first 6000 logits of a 16000-sample clip equal the oracle run on
    the 6000-sample prefix (causality lets the oracle finish in seconds)."""
    from wavenet import WaveNetModel
    T, Tp = 16000, 6000
    cfg = default_cfg(1)
    audio = synth_audio(1, T)
    net = WaveNetModel(seed=0, **model_kwargs(cfg))
    var = {k: v for k, v in _to_numpy(net.variables).items()}
    net.loss(audio, backward=False)
    ws = list(net._ws.values())[0]
    got = ws.logits[:Tp].cpu().numpy()
    q = O.mu_law_encode(audio[:, :Tp], 256)
    ref = O.network_forward(cfg, O.cast_variables(var, np.float64),
                            O.one_hot(q, 256, np.float64))
    assert np.abs(got - ref[0]).max() < 1e-4


def _to_numpy(tree):
    if isinstance(tree, dict):
        return {k: _to_numpy(v) for k, v in tree.items()}
    if isinstance(tree, list):
        return [_to_numpy(v) for v in tree]
    return tree.detach().cpu().numpy()


def make_sine_chord(n=1000, rate=2000.0):
    # test/test_model.py:29-58 (no global conditioning): E-flat chord
    t = np.arange(0.0, n / rate, 1.0 / rate)[:n]
    f1, f2, f3 = 155.56, 196.00, 233.08
    return (np.sin(t * 2 * np.pi * f1) / 3 + np.sin(t * 2 * np.pi * f2) / 3 +
            np.sin(t * 2 * np.pi * f3) / 3).astype(np.float32)


@pytest.mark.parametrize('use_biases', [False, True])
def test_end_to_end_training_thresholds(hip_lib, use_biases):
    """test/test_model.py:179-334 (TestNet / TestNetWithBiases): 14 layers,
    SGD momentum 0.95 lr 0.02, 400 iterations on a 1000-sample chord:
    initial loss > 0.1, final < 0.1, final/initial < 0.02."""
    from wavenet import WaveNetModel, optimizer_factory
    net = WaveNetModel(batch_size=1,
                       dilations=[1, 2, 4, 8, 16, 32, 64] * 2,
                       filter_width=2, residual_channels=32,
                       dilation_channels=32, quantization_channels=256,
                       use_biases=use_biases, skip_channels=32, seed=1)
    audio = make_sine_chord()
    opt = optimizer_factory['sgd'](learning_rate=0.02, momentum=0.95)
    initial = float(net.loss(audio, backward=False))
    for i in range(400):
        loss = net.loss(audio)
        opt.minimize(loss)
    final = float(loss)
    assert initial > 0.1
    assert final < 0.1
    assert final / initial < 0.02


def test_rmsprop_training_then_fast_generation_spectrum(hip_lib):
    """test/test_model.py:337-356 + 137-158: rmsprop lr 1e-3, skip 256; the
    fast-generated waveform carries > 70% of its power at the chord's three
    frequencies."""
    from wavenet import WaveNetModel, optimizer_factory, mu_law_decode
    net = WaveNetModel(batch_size=1, dilations=[1, 2, 4, 8, 16, 32, 64] * 2,
                       filter_width=2, residual_channels=32,
                       dilation_channels=32, quantization_channels=256,
                       skip_channels=256, seed=1)
    audio = make_sine_chord()
    opt = optimizer_factory['rmsprop'](learning_rate=1e-3, momentum=0.95)
    initial = float(net.loss(audio, backward=False))
    for i in range(400):
        loss = net.loss(audio)
        opt.minimize(loss)
    assert float(loss) < 0.1 and float(loss) / initial < 0.02
    codes = net.generate(1000, seed_samples=[128], seed=3)
    wav = mu_law_decode(codes[256:], 256).cpu().numpy()   # skip RF, :91-93
    power = np.abs(np.fft.fft(wav)) ** 2
    freqs = np.fft.fftfreq(wav.size, 1.0 / 2000.0)
    sel = (freqs >= 0) & (freqs <= 500.0)
    power, freqs = power[sel], freqs[sel]
    near = lambda f: power[np.abs(freqs - f).argmin()]
    expected = near(155.56) + near(196.00) + near(233.08)
    assert expected > 0.7 * power.sum()


def test_scalar_input_training_thresholds(hip_lib):
    """test/test_model.py:359-381 (TestNetWithScalarInput): scalar input,
    initial_filter_width 4, sgd lr 0.01, 1000 iterations."""
    from wavenet import WaveNetModel, optimizer_factory
    net = WaveNetModel(batch_size=1, dilations=[1, 2, 4, 8, 16, 32, 64] * 2,
                       filter_width=2, residual_channels=32,
                       dilation_channels=32, quantization_channels=256,
                       use_biases=True, skip_channels=32, scalar_input=True,
                       initial_filter_width=4, seed=1)
    audio = make_sine_chord()
    opt = optimizer_factory['sgd'](learning_rate=0.01, momentum=0.95)
    initial = float(net.loss(audio, backward=False))
    for i in range(1000):
        loss = net.loss(audio)
        opt.minimize(loss)
    final = float(loss)
    assert initial > 0.1 and final < 0.1 and final / initial < 0.02


def test_global_conditioning_training_and_generation(hip_lib):
    """test/test_model.py:384-405 + 159-172 (TestNetWithGlobalConditioning):
    3 speakers, each a different sine; gc_channels = cardinality = 3 (identity
    embedding); after training, the waveform generated (naive windowed path,
    like the reference -- its fast-generation check is commented out,
    test_model.py:293-298) for a speaker carries >= 10x the power at its own
    frequency than at the other two."""
    from wavenet import WaveNetModel, optimizer_factory, mu_law_decode
    rate, n = 2000.0, 1000
    t = np.arange(n) / rate
    freqs = (155.56, 196.00, 233.08)
    amps = (0.6, 0.5, 0.4)
    lead = 64
    audio = np.zeros((3, n), np.float32)
    for i in range(3):
        audio[i, lead:] = amps[i] * np.sin((t[lead:] - t[lead]) * 2 * np.pi * freqs[i])
    ids = np.array([[0], [1], [2]])
    net = WaveNetModel(batch_size=3, dilations=[1, 2, 4, 8, 16, 32, 64] * 2,
                       filter_width=2, residual_channels=32,
                       dilation_channels=32, quantization_channels=256,
                       use_biases=True, skip_channels=256,
                       global_condition_channels=3,
                       global_condition_cardinality=3, seed=1)
    opt = optimizer_factory['sgd'](learning_rate=0.01, momentum=0.95)
    initial = float(net.loss(audio, ids, backward=False))
    for i in range(1000):
        loss = net.loss(audio, ids)
        opt.minimize(loss)
    assert float(loss) < 0.1 and float(loss) / initial < 0.02
    net.batch_size = 1                  # test_model.py:102
    rng = np.random.default_rng(0)
    for spk in range(3):
        # generate_waveform(fast_generation=False), test_model.py:61-95: naive
        # windowed prediction (last 256 samples), host-side np.random.choice
        waveform = [128]
        for i in range(1000):
            window = waveform[-256:]
            p = net.predict_proba(np.asarray(window), [spk]).cpu().numpy()
            p = p.astype(np.float64)
            waveform.append(int(rng.choice(256, p=p / p.sum())))
        wav = mu_law_decode(np.asarray(waveform[256:]), 256).cpu().numpy()
        power = np.abs(np.fft.fft(wav)) ** 2
        fr = np.fft.fftfreq(wav.size, 1.0 / rate)
        sel = (fr >= 0) & (fr <= 500.0)
        power, fr = power[sel], fr[sel]
        near = [power[np.abs(fr - f).argmin()] for f in freqs]
        others = sum(near) - near[spk]
        assert near[spk] > 10.0 * others, (spk, near)


@pytest.mark.parametrize('B,T', [(5, 16000), (8, 16000), (3, 22016)])
def test_three_backward_formulations_many_tiles(hip_lib, B, T):
    """The persistent stack launches (default), the one-launch-per-layer
    kernels (wn_layer_fwd / wn_layer_bwd2: da recomputed per tile, tanh = z /
    sigmoid) and the generic-tap kernel pairs forced on this two-tap model
    (wn_layer_*_k: da planes through memory, tanh plane, separate data and
    weight-gradient launches -- an independent formulation) at tile counts
    above the number of resident waves, dilations below, at and above the
    32-row tile, incl. a clip length with an odd number of tiles, with global
    conditioning (per-tile column sums)."""
    from wavenet import WaveNetModel
    cfg = cfg_with(DEFAULT, batch_size=B, dilations=[1, 32, 64, 512, 2, 256, 16],
                   skip_channels=64, global_condition_channels=4,
                   global_condition_cardinality=5)
    net = WaveNetModel(seed=3, **model_kwargs(cfg))
    audio = synth_audio(B, T)
    ids = np.arange(B) % 5
    res = []
    for stack, generic in ((True, False), (False, False), (False, True)):
        net.stack_fwd = net.stack_bwd = stack
        net.generic_layers = generic
        res.append((float(net.loss(audio, ids)), net.grads.clone()))
    (l0, g0), (l1, g1), (l2, g2) = res
    assert l0 == l1                       # (bitwise the same arithmetic, test_gpu_stack.py)
    assert abs(l2 - l0) <= 1e-6 * abs(l0)
    scale = g2.abs().max().item()
    assert (g1 - g2).abs().max().item() <= 2e-5 * max(scale, 1.0)
    assert (g0 - g2).abs().max().item() <= 2e-5 * max(scale, 1.0)
    # the TN GEMMs on a second stream: same kernels, same slab order -> same bits
    net.stack_fwd = net.stack_bwd = True
    net.generic_layers = False
    net._ws = {}                           # (a workspace with the stack launches' buffers again)
    for ovl in (True, False, True):
        net.overlap_tn = ovl
        for _ in range(3):                 # eager, recorded, replayed plan
            l3 = float(net.loss(audio, ids))
            assert l3 == l0 and torch.equal(net.grads, g0)


@pytest.mark.parametrize('B,expect', [(1, True), (2, True), (3, False)])
def test_small_batch_overlaps_the_weight_gradient_gemms(hip_lib, B, expect):
    """Default stack, T = 16000: with `overlap_tn = None` the three TN GEMMs of
    the skip / post-processing convs run on the side stream next to the
    backward stack when the batch has at most four tiles per CU (B <= 2) --
    same kernels, and at B = 2 the same slab order, so the gradients are the
    bits of the one-stream order (eager, recorded and replayed launch plans)."""
    from wavenet import WaveNetModel
    net = WaveNetModel(seed=4, **model_kwargs(cfg_with(DEFAULT, batch_size=B)))
    audio = synth_audio(B, 16000)
    assert net.overlap_tn is None
    net.overlap_tn = False
    l0 = float(net.loss(audio))
    g0 = net.grads.clone()
    ws = [w for w in net._ws.values() if w.B == B][0]
    assert not net._overlap_tn_on(ws)
    net.overlap_tn = None
    assert net._overlap_tn_on(ws) is expect
    lo, n = net.segments['layers']
    for _ in range(4):
        l1 = float(net.loss(audio))
        assert l1 == l0
        if B > 1:
            assert torch.equal(net.grads, g0)
        else:
            # B = 1: the TN GEMMs beside the stack use 0.6 of the splits (a
            # different, equally fixed summation order for the skip / post-
            # processing weights); everything else is bit-identical
            assert torch.equal(net.grads[lo:lo + n], g0[lo:lo + n])
            scale = g0.abs().max().item()
            assert (net.grads - g0).abs().max().item() <= 2e-6 * scale
    g1 = net.grads.clone()
    net.loss(audio)
    assert torch.equal(net.grads, g1)          # run-to-run identical
