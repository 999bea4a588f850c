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


def _model(B, lc, dilations, R=32, S=64, Q=64, biases=True, gc=None, seed=0,
           D=None, **extra):
    from wavenet import WaveNetModel
    kw = dict(extra)
    if gc:
        kw.update(global_condition_channels=gc, global_condition_cardinality=gc)
    net = WaveNetModel(B, dilations, 2, R, D or R, S, quantization_channels=Q,
                       use_biases=biases, seed=seed,
                       local_condition_channels=lc, **kw)
    if biases:
        _nonzero_biases(net, seed)
    return net


def _nonzero_biases(net, seed):
    # non-zero biases (they start at zero)
    g = torch.Generator().manual_seed(seed + 7)
    with torch.no_grad():
        for n, v in net.named_variables():
            if 'bias' in n.split('/')[-1]:
                v.copy_(0.1 * torch.randn(v.shape, generator=g,
                                          dtype=torch.float64).float())


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


# ---- every launch geometry and model variant against the float64 restatement
# The LC stack launches are their own instantiations (stack_fwd_kernel<SAVE, W,
# StackLc>, stack_bwd_kernel<W, StackLc>), and which W / tiles per wave run
# follows from the number of 32-row tiles B * ceil(T / 32).  Each case below
# asserts the launches it means to cover, through the library's own queries.

_ERRLOG = {}     # case -> (worst gradient error / its bar, variable)


@pytest.fixture(scope='module', autouse=True)
def _dump_errlog():
    """WN_TEST_LOG_DIR set: the observed ratios go to lc_grad_errors.json
    there."""
    yield
    out = os.environ.get('WN_TEST_LOG_DIR')
    if _ERRLOG and out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'lc_grad_errors.json'), 'w') as f:
            json.dump(_ERRLOG, f, indent=1, sort_keys=True)


def _launches(lib, B, T, variant):
    """(tile rows, forward waves, (backward waves, tiles per wave))."""
    import ctypes
    tpw = ctypes.c_int(0)
    bw = lib.wn_stack_bwd_waves(B, T, variant, ctypes.byref(tpw))
    return (lib.wn_stack_tile_rows(B, T, variant),
            lib.wn_stack_fwd_waves(B, T, variant), (bw, tpw.value))


def _find_T(lib, B, T0, variant, fw, bwd):
    """The T nearest T0 (same T mod 32) at which the 32-row launches of a
    (B, T) batch take `fw` forward waves and `bwd` = (waves, tiles per wave)
    backward: the coverage holds whatever CU count the device reports."""
    for k in range(0, 2000):
        for T in (T0 + 32 * k, T0 - 32 * k):
            if T > 0 and _launches(lib, B, T, variant) == (32, fw, bwd):
                return T
    pytest.fail('no T near %d gives forward W %d, backward %s at B = %d'
                % (T0, fw, bwd, B))


def _assert_lc_launches(lib, net, B, T, fw, bwd):
    ws = net._ws[(B, T, True)]
    path = net._step_path(ws, True)
    assert path.fwd == path.bwd == 'stack_lc', path
    assert ws.stack_variant & 0x3f == 32
    assert _launches(lib, B, T, ws.stack_variant) == (32, fw, bwd)


def _check_against_ref(net, dil, codes, lc, ids=None, l2=None, case=None,
                       loss_bar=None, logit_bar=1e-4):
    """One training call and one forward-only call of `net` against
    lc_ref: loss <= 1e-5 relative (or `loss_bar` absolute), every gradient
    <= TOL of its variable's largest entry, logits <= logit_bar.  Returns the
    worst gradient error relative to its bar."""
    B, T = codes.shape
    Q = net.Q
    q = torch.as_tensor(codes).cuda()
    loss = float(net.loss_from_codes(q, ids, l2, local_condition_batch=lc))
    torch.cuda.synchronize()
    ref_loss, ref_g, ref_logits = lc_ref.loss_and_grads(
        lc_ref.model_tree(net), dil, codes, lc, gc_ids=ids,
        use_biases=net.use_biases, quantization_channels=Q,
        relu_masks=lc_ref.device_relu_masks(net, B, T),
        residual_postproc=net.residual_postproc, l2=l2,
        tf_bias_name_quirk=net.tf_bias_name_quirk, return_logits=True)
    if loss_bar is None:
        assert abs(loss - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), \
            (loss, ref_loss)
    else:
        assert abs(loss - ref_loss) < loss_bar, (loss, ref_loss)
    got = dict(lc_ref.flatten(lc_ref.model_tree(net, grads=True)))
    ref = dict(lc_ref.flatten(ref_g))
    assert sorted(got) == sorted(ref)
    worst, bad = (0.0, ''), []
    for k in sorted(ref):
        scale = np.abs(ref[k]).max()
        err = np.abs(got[k] - ref[k]).max()
        worst = max(worst, (float(err / (TOL * max(scale, 1e-30))), k))
        if not err <= TOL * max(scale, 1e-30):
            bad.append((k, float(err), float(scale)))
        if 'lc_' in k:
            assert scale > 0, k
    if case is not None:
        _ERRLOG[case] = worst
    assert not bad, bad[:6]
    loss2 = float(net.loss_from_codes(q, ids, l2, backward=False,
                                      local_condition_batch=lc))
    torch.cuda.synchronize()
    ws = net._ws[(B, T, False)]
    assert net._step_path(ws, False).fwd == 'stack_lc'
    if loss_bar is None:
        assert abs(loss2 - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
    else:
        assert abs(loss2 - ref_loss) < loss_bar
    logits = ws.logits.cpu().numpy().reshape(B, T, -1)
    assert np.abs(logits - ref_logits).max() <= logit_bar
    return worst


DIL10 = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512]

GEOMETRY = [
    # (id, B, T near, variant word (rows, waves) or None, gc, forward W,
    #  (backward W, tiles per wave))
    ('fw2', 2, 4200, None, None, 2, (4, 1)),
    ('fw4_gc', 4, 4200, None, 3, 4, (4, 1)),
    ('fw8', 8, 4200, None, None, 8, (8, 1)),
    ('fw16_tpw2_gc', 8, 8300, None, 4, 16, (8, 2)),
    ('bw1x2', 2, 4200, (32, 1), None, 2, (1, 2)),
    ('bw2x2_gc', 4, 4200, (32, 2), 3, 4, (2, 2)),
    # a variant word asking for 16 rows: an LC model runs 32 (waves kept)
    ('rows16_to_32_bw8', 2, 1000, (16, 8), None, 1, (8, 1)),
]


@pytest.mark.parametrize('case', GEOMETRY, ids=[c[0] for c in GEOMETRY])
def test_every_launch_geometry_matches_float64(hip_lib, case):
    from wavenet import _lib
    name, B, T0, var, gc, fw, bwd = case
    Lc = 80
    net = _model(B, Lc, DIL10, gc=gc, seed=B + fw)
    if var is not None:
        net.stack_variant = _lib.stack_variant(*var)
    v = net._stack_variant_for_launch()
    if var is not None:
        assert v == _lib.stack_variant(32, var[1])
    T = _find_T(hip_lib, B, T0, v, fw, bwd)
    codes, lc = _inputs(B, T, 64, Lc, seed=T)
    ids = None if gc is None else np.arange(B) % gc
    _check_against_ref(net, DIL10, codes, lc, ids, case='%s B%d T%d fw%d bw%dx%d'
                       % (name, B, T, fw, bwd[0], bwd[1]))
    _assert_lc_launches(hip_lib, net, B, T, fw, bwd)


@pytest.mark.parametrize('var', [None, (32, 2)], ids=['library', 'bw2'])
@pytest.mark.parametrize('B,T', [(2, 333), (8, 301)])
def test_unaligned_dilations_match_float64(hip_lib, B, T, var):
    """DIL_A (tests/util.py; tests/test_dilations_host.py counts what it
    reaches at T = 333 and 301): taps that straddle two foreign tiles, taps
    that start inside a later tile, rows t + d cut by the clip's end -- in the
    LC instantiations of the stack launches, at the library's launch choice
    and with two backward waves per workgroup."""
    from util import DIL_A
    from wavenet import _lib
    Lc = 80
    net = _model(B, Lc, DIL_A, seed=B + T)
    if var is not None:
        net.stack_variant = _lib.stack_variant(*var)
    v = net._stack_variant_for_launch()
    rows, fw, bwd = _launches(hip_lib, B, T, v)
    assert rows == 32 and (var is None or bwd[0] == var[1])
    codes, lc = _inputs(B, T, 64, Lc, seed=T)
    _check_against_ref(net, DIL_A, codes, lc, case='dil_A B%d T%d fw%d bw%dx%d'
                       % (B, T, fw, bwd[0], bwd[1]))
    _assert_lc_launches(hip_lib, net, B, T, fw, bwd)


def test_default_stack_takes_the_lc_launches_not_stack_skip(hip_lib):
    """wavenet_params.json (L = 50, S = 512, Q = 256) at 2 x 5200: without LC
    the fused-skip forward (which ignores LC) would cover this shape."""
    from wavenet import WaveNetModel
    from util import model_kwargs
    params = json.load(open(os.path.join(ROOT, 'wavenet_params.json')))
    params['batch_size'] = 2
    B, Lc = 2, 80
    net = WaveNetModel(seed=3, local_condition_channels=Lc,
                       **model_kwargs(params))
    _nonzero_biases(net, 3)
    v = net._stack_variant_for_launch()
    T = _find_T(hip_lib, B, 5200, v, 2, (4, 1))
    codes, lc = _inputs(B, T, net.Q, Lc, seed=11)
    # (the same shape without LC: 16-row tiles and the fused skip sum)
    assert hip_lib.wn_stack_fwd_skip_ok(B, T, net.S, net.stack_variant) == 1
    _check_against_ref(net, params['dilations'], codes, lc,
                       case='default_stack B%d T%d fw2 bw4x1' % (B, T))
    _assert_lc_launches(hip_lib, net, B, T, 2, (4, 1))
    assert not net._ws[(B, T, True)].fwd_skip_ok


DIL_V = [1, 2, 4, 8, 16, 32, 64, 128, 1, 2]

VARIANTS = [
    # (id, model kwargs, Lc, gc, l2)
    ('r16_lc5', dict(R=16), 5, None, None),
    ('r24_d20_lc5_gc', dict(R=24, D=20), 5, 3, None),
    ('residual_postproc', dict(residual_postproc=True), 16, None, None),
    ('l2_quirk', dict(), 16, None, 0.05),
    ('l2_no_quirk_gc', dict(tf_bias_name_quirk=False), 16, 3, 0.05),
    ('bf16x6', dict(gemm_mode='bf16x6'), 80, None, None),
    ('bf16x9_gc', dict(gemm_mode='bf16x9'), 80, 3, None),
    ('lc300', dict(), 300, None, None),
]


@pytest.mark.parametrize('case', VARIANTS, ids=[c[0] for c in VARIANTS])
def test_model_variants_match_float64(hip_lib, case):
    name, kw, Lc, gc, l2 = case
    kw = dict(kw)
    B, T = 2, 700
    attrs = {k: kw.pop(k) for k in ('gemm_mode', 'tf_bias_name_quirk')
             if k in kw}
    net = _model(B, Lc, DIL_V, gc=gc, seed=Lc, **kw)
    for k, val in attrs.items():
        setattr(net, k, val)
    assert net.Lcp == -(-Lc // 4) * 4
    codes, lc = _inputs(B, T, 64, Lc, seed=Lc + 1)
    ids = None if gc is None else np.arange(B) % gc
    # (gemm_mode: the bars of test_gpu_model.py's split-bf16 parity test)
    split = 'gemm_mode' in attrs
    _check_against_ref(net, DIL_V, codes, lc, ids, l2=l2, case=name,
                       loss_bar=1e-4 if split else None)
    if split:
        assert net._wsplit, 'split path not taken'
    _assert_lc_launches(hip_lib, net, B, T, 1, (4, 1))


def test_lc_weight_padding_stays_zero_through_adam(hip_lib):
    """R = D = 16, Lc = 5: lc_w is [Lcp = 8][L][64] with filter columns 0..15
    and gate columns 32..47.  After three Adam steps the padding -- rows 5..7,
    columns 16..31 and 48..63 -- is exactly zero in the parameters and the
    gradients, and the real entries moved."""
    from wavenet import optimizer_factory
    B, T, Lc, D = 2, 700, 5, 16
    net = _model(B, Lc, DIL_V, R=D, seed=9)
    L = net.L
    view = lambda t: net._seg(t, 'lc_w').view(net.Lcp, L, 64)
    before = view(net.params).clone()
    opt = optimizer_factory['adam'](learning_rate=1e-2, momentum=0.9)
    for s in range(3):
        codes, lc = _inputs(B, T, 64, Lc, seed=20 + s)
        loss = net.loss_from_codes(torch.as_tensor(codes).cuda(),
                                   local_condition_batch=lc)
        opt.minimize(loss)
    torch.cuda.synchronize()
    for t in (view(net.params), view(net.grads)):
        t = t.cpu()
        assert int(torch.count_nonzero(t[Lc:])) == 0
        assert int(torch.count_nonzero(t[:, :, D:32])) == 0
        assert int(torch.count_nonzero(t[:, :, 32 + D:])) == 0
    p = view(net.params).cpu()
    moved = (p != before.cpu())
    assert bool(moved[:Lc, :, :D].all()) and bool(moved[:Lc, :, 32:32 + D].all())


def test_predict_proba_matches_float64_in_carved_workspaces(hip_lib):
    """predict_proba (the forward-only SAVE = 0 launch) with LC on one B = 1
    net: first T = 3000, then shorter T whose workspaces are carved out of
    the first (as naive generation does).  Each answer is the softmax of the
    float64 logits at row T - 1 (causal: the rows of the full restatement)."""
    B, Tmax, Lc = 1, 3000, 12
    dil = [1, 2, 4, 8, 16, 32, 64, 128, 256]
    net = _model(B, Lc, dil, gc=3, seed=4)
    codes, lc = _inputs(B, Tmax, 64, Lc, seed=6)
    ids = [2]
    ref = lc_ref.logits(lc_ref.model_tree(net), dil, codes, lc, gc_ids=ids,
                        use_biases=True, quantization_channels=64)[0]
    for i, T in enumerate((Tmax, 2999, 2048, 1000, 257, 40)):
        p = net.predict_proba(codes[:, :T], ids,
                              local_condition=lc[:, :T]).cpu().numpy()
        ws = net._ws[(B, T, False)]
        assert (ws.capacity == ws.N) == (i == 0)        # carved after the first
        assert net._step_path(ws, False).fwd == 'stack_lc'
        r = ref[T - 1]
        want = np.exp(r - r.max())
        want /= want.sum()
        assert np.abs(p.astype(np.float64) - want).max() <= 1e-5, T


def test_launch_plan_replay_with_new_lc_values(hip_lib):
    """Three training calls on one net -- eager, recorded and replayed launch
    plans -- each with new codes, GC ids and non-zero LC: every one matches
    lc_ref for its own inputs."""
    B, T, Lc = 2, 900, 24
    dil = [1, 2, 4, 8, 16, 32, 64, 128]
    net = _model(B, Lc, dil, gc=3, seed=8)
    assert net.use_launch_plans
    for s in range(3):
        codes, lc = _inputs(B, T, 64, Lc, seed=100 + s)
        ids = np.array([s % 3, (s + 1) % 3])
        _check_against_ref(net, dil, codes, lc, ids, case='replay call %d' % s)
    ws = net._ws[(B, T, True)]
    assert any(isinstance(p, list) and len(p) > 5 for p in ws.plans.values())
