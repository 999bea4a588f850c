"""Local conditioning on the GPU: loss and every gradient against the float64
restatement (tests/lc_ref.py), all-zero LC bitwise equal to the model without
LC, causality / alignment of the conditioning rows, learning from LC, the
fast-generation refusals and train.py / generate.py end to end."""
import json
import os
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import lc_ref
from util import ROOT

sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

TOL = 2e-5     # of each variable's largest entry (the project's bar)


def _model(B, lc, dilations, R=32, S=64, Q=64, biases=True, gc=None, seed=0):
    from wavenet import WaveNetModel
    kw = {}
    if gc:
        kw = dict(global_condition_channels=gc, global_condition_cardinality=gc)
    net = WaveNetModel(B, dilations, 2, R, R, S, quantization_channels=Q,
                       use_biases=biases, seed=seed,
                       local_condition_channels=lc, **kw)
    if biases:
        # non-zero biases (they start at zero)
        g = torch.Generator().manual_seed(seed + 7)
        with torch.no_grad():
            for n, v in net.named_variables():
                if 'bias' in n.split('/')[-1]:
                    v.copy_(0.1 * torch.randn(v.shape, generator=g,
                                              dtype=torch.float64).float())
    return net


def _inputs(B, T, Q, Lc, seed=0):
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, Q, (B, T)).astype(np.int32)
    lc = rng.standard_normal((B, T, Lc)).astype(np.float32) if Lc else None
    return codes, lc


CASES = [
    # (biases, gc, Lc, B, T, dilations)
    (True, 4, 80, 8, 300, [1, 2, 4, 8, 16, 32, 64]),
    (False, None, 80, 8, 300, [1, 2, 4, 8, 16, 32, 64]),
    (True, None, 1, 1, 700, [1, 2, 4, 8, 16, 32, 64, 128, 256]),
    (False, 3, 200, 1, 450, [1, 64, 2, 128, 4, 33]),
    (True, None, 200, 8, 160, [1, 2, 4, 8, 16, 32, 64, 128]),
]


@pytest.mark.parametrize('case', CASES,
                         ids=['b_gc_lc80_B8', 'nob_lc80_B8', 'b_lc1_B1_long',
                              'nob_gc_lc200_B1', 'b_lc200_B8'])
def test_loss_and_gradients_match_float64(hip_lib, case):
    biases, gc, Lc, B, T, dil = case
    Q = 64
    net = _model(B, Lc, dil, biases=biases, gc=gc, seed=len(dil))
    codes, lc = _inputs(B, T, Q, Lc, seed=B + Lc)
    ids = None if gc is None else np.arange(B) % gc
    loss = net.loss_from_codes(torch.as_tensor(codes).cuda(),
                               global_condition_batch=ids,
                               local_condition_batch=lc)
    torch.cuda.synchronize()
    ref_loss, ref_g = lc_ref.loss_and_grads(
        lc_ref.model_tree(net), dil, codes, lc, gc_ids=ids, use_biases=biases,
        quantization_channels=Q, relu_masks=lc_ref.device_relu_masks(net, B, T))
    assert abs(float(loss) - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
    got = dict(lc_ref.flatten(lc_ref.model_tree(net, grads=True)))
    ref = dict(lc_ref.flatten(ref_g))
    assert sorted(got) == sorted(ref)
    assert any('lc_filtweights' in k for k in got)
    for k in sorted(ref):
        scale = np.abs(ref[k]).max()
        err = np.abs(got[k] - ref[k]).max()
        assert err <= TOL * max(scale, 1e-30), (k, err, scale)
    for k in ref:
        if k.endswith('lc_filtweights') or k.endswith('lc_gateweights'):
            assert np.abs(ref[k]).max() > 0, k


def test_all_zero_lc_is_bitwise_the_model_without_lc(hip_lib):
    from wavenet import _lib
    B, T, dil = 2, 1000, [1, 2, 4, 8, 16, 32, 64, 128, 1, 2]
    net_lc = _model(B, 80, dil, gc=3, seed=5)
    net = _model(B, None, dil, gc=3, seed=5)
    # (at this B the model without LC would take the 16-row launches)
    net.stack_variant = _lib.stack_variant(rows=32)
    shared = [n for n, _ in net.named_variables()]
    vl = dict(net_lc.named_variables())
    for n, v in net.named_variables():
        assert torch.equal(v, vl[n]), n
    codes, _ = _inputs(B, T, 64, 0, seed=1)
    zeros = np.zeros((B, T, 80), np.float32)
    ids = [0, 2]
    q = torch.as_tensor(codes).cuda()
    for _ in range(2):      # (the second call replays the recorded launch plan)
        a = net_lc.loss_from_codes(q, ids, local_condition_batch=zeros)
        b = net.loss_from_codes(q, ids)
        torch.cuda.synchronize()
        assert float(a) == float(b)
        gl = dict(net_lc.named_variables(net_lc.gradients))
        for n, g in net.named_variables(net.gradients):
            assert torch.equal(g, gl[n]), n
        for n in gl:
            if n not in shared:
                assert 'lc_' in n and int(torch.count_nonzero(gl[n])) == 0, n


def test_lc_is_causal_and_row_t_conditions_output_t(hip_lib):
    B, T, t0, Lc = 1, 600, 377, 5
    dil = [1, 2, 4, 8, 16, 32, 64, 128]
    net = _model(B, Lc, dil, seed=2)
    codes, lc = _inputs(B, T, 64, Lc, seed=4)
    lc2 = lc.copy()
    lc2[:, t0:] += 1.0
    out = []
    for x in (lc, lc2):
        p = net.predict_proba(codes, local_condition=x)
        ws = net._ws[(B, T, False)]
        out.append((p.cpu().numpy(), ws.logits.cpu().numpy().copy()))
    torch.cuda.synchronize()
    la, lb = out[0][1], out[1][1]
    assert np.array_equal(la[:t0], lb[:t0])
    assert not np.array_equal(la[t0], lb[t0])
    assert (np.abs(la[t0:] - lb[t0:]).max(axis=1) > 0).all()
    # predict_proba's answer is the distribution after the last sample, which
    # the last row conditions
    assert not np.array_equal(out[0][0], out[1][0])


def _learning_run(with_lc, steps=300):
    from wavenet import optimizer_factory
    B, T, K, Q = 4, 256, 4, 16
    net = _model(B, K if with_lc else None, [1, 2, 4, 8], R=16, S=32, Q=Q,
                 biases=True, seed=1)
    opt = optimizer_factory['adam'](learning_rate=0.01, momentum=0.9)
    rng = np.random.default_rng(0)
    loss = None
    for step in range(steps):
        cls = rng.integers(0, K, (B, T))
        lc = np.eye(K, dtype=np.float32)[cls]
        codes = np.empty((B, T), np.int32)
        codes[:, 0] = 0
        codes[:, 1:] = 3 * cls[:, :-1] + 1     # sample t + 1 is a function of lc row t
        loss = net.loss_from_codes(
            torch.as_tensor(codes).cuda(),
            local_condition_batch=lc if with_lc else None)
        opt.minimize(loss)
    return float(loss)


def test_learns_from_lc(hip_lib):
    plain = _learning_run(False)
    cond = _learning_run(True)
    # without LC the next code is a uniform pick of four: about log 4 = 1.39
    assert plain > 1.0, plain
    assert cond < 0.2 * plain, (cond, plain)


def test_fast_generation_refuses_lc_models(hip_lib):
    net = _model(1, 8, [1, 2, 4, 8], seed=0)
    calls = [lambda: net.generate(10),
             lambda: net.predict_proba_incremental([3]),
             lambda: net.prime_generator([1, 2, 3]),
             lambda: net.continue_generation(4, 3),
             lambda: net.generate_batch(4, [1, 2]),
             lambda: net.continue_generation_batch(4, [1, 2], [1, 2])]
    for c in calls:
        with pytest.raises(NotImplementedError, match='predict_proba'):
            c()


SMALL = {"filter_width": 2, "sample_rate": 16000,
         "dilations": [1, 2, 4, 8, 16, 32, 1, 2, 4, 8, 16, 32],
         "residual_channels": 32, "dilation_channels": 32,
         "quantization_channels": 256, "skip_channels": 64,
         "use_biases": True, "scalar_input": False,
         "initial_filter_width": 32, "residual_postproc": False}


def test_train_and_naive_generation_with_lc(hip_lib, tmp_path, capsys):
    import generate
    import train
    params = str(tmp_path / 'params.json')
    json.dump(SMALL, open(params, 'w'))
    logdir = str(tmp_path / 'run')
    assert train.main(['--synthetic', '--lc_channels', '80', '--lc_hop', '4',
                       '--sample_size', '2000', '--batch_size', '2',
                       '--wavenet_params', params, '--logdir', logdir,
                       '--checkpoint_every', '3', '--num_steps', '4',
                       '--learning_rate', '0.002']) == 0
    out = capsys.readouterr().out
    assert 'step 3 - loss = ' in out
    ck = train.latest_checkpoint(logdir)
    assert ck.endswith('model.ckpt-3')
    sd = torch.load(ck, map_location='cpu')['variables']
    assert tuple(sd['wavenet/dilated_stack/layer0/lc_filter'].shape) == (80, 32)
    hop, frames = 3, 50
    feats = np.random.default_rng(0).standard_normal((frames, 80)).astype(
        np.float32)
    np.save(str(tmp_path / 'f.npy'), feats)
    wav = str(tmp_path / 'out.wav')
    assert generate.main([ck, '--wavenet_params', params, '--fast_generation',
                          'false', '--lc_path', str(tmp_path / 'f.npy'),
                          '--lc_hop', str(hop), '--wav_out_path', wav,
                          '--logdir', str(tmp_path / 'gen')]) == 0
    rate, data = wavfile.read(wav)
    # the one seed sample + one sample per upsampled feature row
    assert rate == 16000 and data.shape == (1 + hop * frames,)
    assert np.isfinite(data).all()
    # fast generation refuses LC with a pointer to the naive path
    assert generate.main([ck, '--wavenet_params', params, '--lc_path',
                          str(tmp_path / 'f.npy')]) == 1
    assert '--fast_generation false' in capsys.readouterr().out
