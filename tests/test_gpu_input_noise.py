"""Input noise on the GPU (wavenet/input_noise.py, csrc/wn_misc.hip's
code_noise_kernel, `input_codes` / `input_noise` on the loss and the score):

  1. both kernels bit for bit against the Python-integer restatement of
     tests/noise_ref.py over its grid of shapes and settings, the clamps,
     out-of-range codes, unaligned buffers, the fused kernel's clean output
     against ops.mu_law_encode;
  2. input_codes = q and prob = 0 give the bits of the call without them;
  3. loss and every gradient with perturbed inputs and clean targets against
     float64 (tests/noise_ref.py on tests/lc_ref.py's network);
  4. the score with perturbed inputs against float64;
  5. train.py --input_noise and evaluate.py --input_noise end to end.

Bars: those of tests/test_gpu_masked_loss.py -- the loss within 1e-5 relative,
every gradient within TOL = 2e-5 of its variable's largest entry -- and of
tests/test_gpu_score.py -- nll / count within 1e-5 relative of max(1, |ref|),
counts exact, `correct` bound by the rows whose float64 top-two margin exceeds
1e-3.  dlogits: the project's bar on fp32 logits is 1e-4 absolute, and an
entry (softmax - one_hot) / D moves at most half as far as its logits: 1e-4 / D
absolute."""
import json
import os
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import lc_ref
import noise_ref as R
import score_ref
from util import ROOT, TINY, cfg_with, model_kwargs

sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

TOL = 2e-5     # of each variable's largest entry (the project's bar)
FAR = 100      # "far more than the bar": this many bars


def _noise(*a):
    from wavenet.input_noise import InputNoise
    return InputNoise(*a)


def _dev(x):
    return torch.as_tensor(np.asarray(x)).cuda()


# ---- 1. the kernels, bit for bit --------------------------------------------
def test_both_kernels_match_the_restatement_over_the_grid(hip_lib):
    from wavenet.ops import mu_law_encode
    n, clean = 0, {}
    for audio, q, keys, lengths, Q, prob, width, seed in R.grid():
        f = _noise(prob, width, seed)
        want = R.codes_in(q, keys, lengths, Q, prob, width, seed)
        what = (q.shape, keys.tolist(), lengths, Q, prob, width, seed)
        got = f.codes(q, keys, lengths, Q=Q)
        assert got.dtype == torch.int32 and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), want), what
        if (q.shape, Q) not in clean:       # (one audio per shape and Q)
            clean[q.shape, Q] = mu_law_encode(audio, Q).cpu().numpy()
            assert np.array_equal(clean[q.shape, Q], q)     # oracle's codes
        c, ci = f.encode(audio, Q, keys, lengths)
        assert np.array_equal(c.cpu().numpy(), clean[q.shape, Q]), what
        assert np.array_equal(ci.cpu().numpy(), want), what
        n += 1
    assert n == 1008


def test_clamps_out_of_range_codes_and_unaligned_buffers(hip_lib):
    rng = np.random.default_rng(3)
    keys = np.array([0, (1 << 40) - 1, 77], np.int64)
    for Q in (16, 256):
        for B, T in ((3, 1027), (2, 1024)):
            k = keys[:B]
            # only the two edge codes: every move is clamped on one side
            edge = np.where(rng.random((B, T)) < 0.5, 0,
                            Q - 1).astype(np.int32)
            for width in (1, Q - 1):
                got = _noise(1, width, 5).codes(edge, k, Q=Q).cpu().numpy()
                assert np.array_equal(
                    got, R.codes_in(edge, k, None, Q, 1.0, width, 5))
                assert got.min() == 0 and got.max() == Q - 1
                assert (got != edge).any()
            # one code out of range each way passes through
            q = rng.integers(0, Q, (B, T)).astype(np.int32)
            q[0, 5], q[B - 1, T - 2] = -1, Q
            n = [T, 501, 1][:B]
            got = _noise(1, 3, 9).codes(q, k, n, Q=Q).cpu().numpy()
            assert np.array_equal(got, R.codes_in(q, k, n, Q, 1.0, 3, 9))
            assert got[0, 5] == -1 and got[B - 1, T - 2] == Q
            # buffers 4 bytes off a 16-byte boundary, in place, device keys
            want = R.codes_in(q, k, None, Q, 0.5, 3, 9)
            flat = torch.zeros(B * T + 1, dtype=torch.int32, device='cuda')
            src = flat[1:].view(B, T)
            src.copy_(_dev(q))
            assert src.data_ptr() % 16 == 4
            f = _noise(0.5, 3, 9)
            assert np.array_equal(f.codes(src, k, Q=Q).cpu().numpy(), want)
            out = f.codes(src, _dev(k), Q=Q, out=src)
            assert out is src and np.array_equal(src.cpu().numpy(), want)
            assert int(flat[0]) == 0


def test_fused_kernel_is_encode_then_noise(hip_lib):
    from wavenet.ops import mu_law_encode
    rng = np.random.default_rng(4)
    for B, T, Q in ((3, 1027, 256), (2, 4099, 16), (1, 7, 256)):
        a = rng.uniform(-1.2, 1.2, (B, T)).astype(np.float32)   # also |x| > 1
        a[0, :4] = (-1.0, 1.0, 0.0, -0.0)
        keys = np.arange(B, dtype=np.int64) + 9
        n = [T, 3, 1][:B]
        f = _noise(0.5, 3, 1 << 63)
        ad = _dev(a)
        q, q_in = f.encode(ad, Q, keys, n)
        clean = mu_law_encode(ad, Q)
        assert torch.equal(q, clean)
        assert torch.equal(q_in, f.codes(clean, keys, n, Q=Q))
        assert np.array_equal(q_in.cpu().numpy(), R.codes_in(
            clean.cpu().numpy(), keys, n, Q, 0.5, 3, 1 << 63))
        # into given buffers; nothing else is written
        flat = torch.full((2 * B * T + 2,), -7, dtype=torch.int32,
                          device='cuda')
        o0, o1 = flat[:B * T].view(B, T), flat[B * T + 1:-1].view(B, T)
        r0, r1 = f.encode(ad, Q, keys, n, out=(o0, o1))
        assert r0 is o0 and r1 is o1
        assert torch.equal(o0, q) and torch.equal(o1, q_in)
        assert int(flat[B * T]) == -7 and int(flat[-1]) == -7


# ---- models -----------------------------------------------------------------
def _net(cfg, rows=None, seed=0, **extra):
    from wavenet import WaveNetModel, _lib
    net = WaveNetModel(seed=seed, **model_kwargs(cfg), **extra)
    g = torch.Generator().manual_seed(seed + 7)
    with torch.no_grad():
        for n, v in net.named_variables():
            if 'bias' in n.split('/')[-1]:
                v.copy_(0.1 * torch.randn(v.shape, generator=g,
                                          dtype=torch.float64).float())
    if rows is not None:
        net.stack_variant = _lib.stack_variant(rows=rows)
    return net


def _codes(B, T, Q, seed):
    return np.random.default_rng(seed).integers(0, Q, (B, T)).astype(np.int32)


def _bucket(net):
    torch.cuda.synchronize()
    return net.grads.clone()


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64
                               else torch.int32)


# ---- 2. identities ----------------------------------------------------------
def test_input_codes_equal_to_the_codes_change_no_bit(hip_lib):
    B, T = 2, 250
    cfg = cfg_with(TINY, batch_size=B, global_condition_channels=4,
                   global_condition_cardinality=3)
    net = _net(cfg)
    q = _dev(_codes(B, T, net.Q, 1))
    ids = [2, 0]
    for _ in range(3):              # eager, recorded, replayed
        for kw in (dict(), dict(lengths=[T, 141]),
                   dict(lengths=[T, 141], history=[9, 0])):
            a = net.loss_from_codes(q, ids, **kw).clone()
            ga = _bucket(net)
            b = net.loss_from_codes(q, ids, input_codes=q.clone(),
                                    **kw).clone()
            gb = _bucket(net)
            assert torch.equal(a, b), (float(a), float(b))
            assert torch.equal(ga, gb) and float(ga.abs().max()) > 0
            sa = net.score_from_codes(q, ids, per_sample=True, **kw)
            sb = net.score_from_codes(q, ids, per_sample=True,
                                      input_codes=q.clone(), **kw)
            for name, x, y in zip(sa._fields, sa, sb):
                assert torch.equal(_bits(x), _bits(y)), name
            assert float(sa.nll.abs().max()) > 0


def test_prob_zero_changes_no_bit(hip_lib):
    B, T = 2, 233
    net = _net(cfg_with(TINY, batch_size=B))
    audio = np.random.default_rng(2).uniform(-1, 1, (B, T)).astype(np.float32)
    f, keys = _noise(0, 3, 11), np.array([4, (1 << 40) - 1])
    for _ in range(3):
        for kw in (dict(), dict(lengths=[77, T])):
            a = net.loss(audio, **kw).clone()
            ga = _bucket(net)
            b = net.loss(audio, input_noise=f, noise_keys=keys, **kw).clone()
            gb = _bucket(net)
            assert torch.equal(a, b) and torch.equal(ga, gb)
            assert float(ga.abs().max()) > 0
            sa = net.score(audio, per_sample=True, **kw)
            sb = net.score(audio, per_sample=True, input_noise=f,
                           noise_keys=keys, **kw)
            for name, x, y in zip(sa._fields, sa, sb):
                assert torch.equal(_bits(x), _bits(y)), name


# ---- 3. perturbed inputs, clean targets, against float64 --------------------
def _rel(got, ref):
    """(worst error of a gradient tree in units of its variable's largest
    reference entry, that variable)."""
    got, ref = dict(lc_ref.flatten(got)), dict(lc_ref.flatten(ref))
    assert sorted(got) == sorted(ref)
    return max((np.abs(got[k] - ref[k]).max() /
                max(np.abs(ref[k]).max(), 1e-30), k) for k in ref)


def _assert_close(tag, loss, grads, ref_loss, ref_g):
    print('%s: loss %.9g reference %.9g relative error %.3g'
          % (tag, loss, ref_loss,
             abs(loss - ref_loss) / max(1.0, abs(ref_loss))))
    worst = _rel(grads, ref_g)
    print('%s: worst gradient error %.3g of the largest entry (%s), bar %g'
          % (tag, worst[0], worst[1], TOL))
    assert abs(loss - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
    ref = dict(lc_ref.flatten(ref_g))
    got = dict(lc_ref.flatten(grads))
    assert max(np.abs(a).max() for a in ref.values()) > 0
    for k in sorted(ref):
        scale = np.abs(ref[k]).max()
        err = np.abs(got[k] - ref[k]).max()
        assert err <= TOL * max(scale, 1e-30), (tag, k, err, scale)


BLOCKED = cfg_with(TINY, residual_channels=64, dilation_channels=64,
                   skip_channels=32, quantization_channels=64)
GC = dict(global_condition_channels=4, global_condition_cardinality=3)
# (name, configuration, model extras, T, tile rows asked / expected, call
#  keywords)
CASES = [
    ('tiny_rows16', TINY, {}, 250, None, 16, {}),
    ('tiny_rows32', TINY, {}, 231, 32, 32, {}),
    ('tiny_gc', cfg_with(TINY, **GC), {}, 200, None, 16, {}),
    ('tiny_lc4', TINY, dict(local_condition_channels=4), 263, None, None, {}),
    ('tiny_k3', cfg_with(TINY, filter_width=3), {}, 210, None, None, {}),
    ('blocked64', BLOCKED, {}, 200, None, None, {}),
    ('tiny_lengths_history', TINY, {}, 300, None, 16,
     dict(lengths=[300, 141], history=[20, 0])),
]


@pytest.mark.parametrize('name, cfg, extra, T, rows, want_rows, kw', CASES,
                         ids=[c[0] for c in CASES])
def test_noisy_inputs_clean_targets_match_float64(hip_lib, name, cfg, extra,
                                                  T, rows, want_rows, kw):
    B = 2
    cfg = cfg_with(cfg, batch_size=B)
    net = _net(cfg, rows=rows, seed=T, **extra)
    Q, Lc = net.Q, extra.get('local_condition_channels')
    rng = np.random.default_rng(T)
    codes = _codes(B, T, Q, T)
    lc = rng.standard_normal((B, T, Lc)).astype(np.float32) if Lc else None
    ids = [2, 0] if 'global_condition_channels' in cfg else None
    keys = np.array([T, (1 << 40) - 1], np.int64)
    f = _noise(0.5, 2, 1234)
    lengths = kw.get('lengths')
    q = _dev(codes)
    q_in = f.codes(q, keys, lengths, Q=Q)
    want_in = R.codes_in(codes, keys, lengths, Q, 0.5, 2, 1234)
    assert np.array_equal(q_in.cpu().numpy(), want_in)
    moved = (want_in != codes).mean()
    assert 0.1 < moved < 0.5, moved
    call = dict(local_condition_batch=lc, **kw)
    # the clean call, for the separation below
    net.loss_from_codes(q, ids, **call)
    torch.cuda.synchronize()
    g_clean = lc_ref.model_tree(net, grads=True)
    ws = net._ws[(B, T, True)]
    dl_clean = ws.logits.reshape(B, T, Q).cpu().numpy().astype(np.float64)
    loss = float(net.loss_from_codes(q, ids, input_codes=q_in, **call))
    torch.cuda.synchronize()
    assert ws is net._ws[(B, T, True)]
    if want_rows is not None:
        assert ws.stack_bwd and ws.stack_rows == want_rows
    if cfg is not None and cfg['residual_channels'] > 32:
        assert net.blocked
    grads = lc_ref.model_tree(net, grads=True)
    dl = ws.logits.reshape(B, T, Q).cpu().numpy().astype(np.float64)
    ref_loss, ref_g, raw = R.loss_and_grads(
        lc_ref.model_tree(net), cfg['dilations'], codes, want_in, lc,
        gc_ids=ids, lengths=lengths, history=kw.get('history'),
        use_biases=net.use_biases, quantization_channels=Q,
        relu_masks=lc_ref.device_relu_masks(net, B, T), return_logits=True)
    _assert_close(name, loss, grads, ref_loss, ref_g)
    # forward only: the same loss
    fwd = float(net.loss_from_codes(q, ids, backward=False,
                                    input_codes=q_in, **call))
    assert abs(fwd - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
    # the test can tell the two calls apart: far more than the bar
    sep = _rel(g_clean, ref_g)
    print('%s: the clean call\'s gradients are %.3g of the largest entry off '
          '(%s)' % (name, sep[0], sep[1]))
    assert sep[0] > FAR * TOL
    # ... and the targets are the clean codes: dlogits = (softmax - one_hot of
    # the CLEAN next code) / D on rows with a target
    if not kw:
        D = float(B * T)
        p = np.exp(raw - raw.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        def expected(targets):
            e = p.copy()
            e[:, :-1] -= np.eye(Q)[targets[:, 1:]]
            return e / D
        err = np.abs(dl - expected(codes)).max()
        off = np.abs(dl - expected(want_in)).max()
        print('%s: dlogits %.3g off the clean targets\' (bar %.3g), %.3g off '
              'the perturbed targets\'' % (name, err, 1e-4 / D, off))
        assert err <= 1e-4 / D
        assert off > FAR * 1e-4 / D
        assert np.abs(dl - dl_clean).max() > FAR * 1e-4 / D


def test_loss_with_input_noise_is_the_loss_on_its_codes(hip_lib):
    """loss(audio, input_noise=...) through the fused kernel == loss_from_codes
    (q, input_codes=codes(q)), bit for bit, with lengths and history; and a
    replayed launch sees the call's keys."""
    from wavenet.ops import mu_law_encode
    B, T = 2, 250
    net = _net(cfg_with(TINY, batch_size=B))
    audio = _dev(np.random.default_rng(5).uniform(-1, 1, (B, T))
                 .astype(np.float32))
    q = mu_law_encode(audio, net.Q)
    f = _noise(0.5, 2, 3)
    seen = set()
    for step in range(4):
        keys = np.array([2 * step, 2 * step + 1], np.int64)
        for kw in (dict(), dict(lengths=[T, 99], history=[0, 30])):
            a = net.loss(audio, input_noise=f, noise_keys=keys, **kw).clone()
            ga = _bucket(net)
            q_in = f.codes(q, keys, kw.get('lengths'), Q=net.Q)
            b = net.loss_from_codes(q, input_codes=q_in, **kw).clone()
            assert torch.equal(a, b) and torch.equal(ga, _bucket(net))
            sa = net.score(audio, input_noise=f, noise_keys=keys, **kw)
            sb = net.score_from_codes(q, input_codes=q_in, **kw)
            assert torch.equal(_bits(sa.nll), _bits(sb.nll))
            assert torch.equal(sa.correct, sb.correct)
            seen.add(float(a))
    assert len(seen) == 8           # other keys, other draws, another loss


# ---- 4. the score -----------------------------------------------------------
def test_score_with_input_codes_matches_float64(hip_lib):
    B, T = 2, 250
    cfg = cfg_with(TINY, batch_size=B)
    net = _net(cfg, seed=4)
    Q = net.Q
    codes = _codes(B, T, Q, 8)
    keys = np.array([1, 2], np.int64)
    f = _noise(0.5, 2, 1234)
    for lengths in (None, [T, 141]):
        want_in = R.codes_in(codes, keys, lengths, Q, 0.5, 2, 1234)
        q_in = f.codes(codes, keys, lengths, Q=Q)
        s = net.score_from_codes(_dev(codes), input_codes=q_in,
                                 lengths=lengths, per_sample=True)
        torch.cuda.synchronize()
        ref = R.logits(lc_ref.model_tree(net), cfg['dilations'], want_in,
                       use_biases=net.use_biases, quantization_channels=Q)
        r = score_ref.rows(ref, codes, lengths, Q)
        ref_nll, ref_cnt, _ = score_ref.clips(r)
        nll, cnt = s.nll.cpu().numpy(), s.count.cpu().numpy()
        cor = s.correct.cpu().numpy()
        n = np.full(B, T) if lengths is None else np.asarray(lengths)
        assert cnt.tolist() == (n - 1).tolist() == ref_cnt.tolist()
        ps = s.per_sample.cpu().numpy().astype(np.float64)
        err = np.abs(ps - r['nll']).max()
        print('lengths %s: worst per_sample error %.3g (bar 2e-4)'
              % (lengths, err))
        assert err <= 2e-4 and (ps[~r['has']] == 0.0).all()
        for b in range(B):
            got, want = nll[b] / cnt[b], ref_nll[b] / ref_cnt[b]
            print('lengths %s: clip %d nll/count %.9g reference %.9g'
                  % (lengths, b, got, want))
            assert abs(got - want) <= 1e-5 * max(1.0, abs(want))
        sure = r['has'] & (r['margin'] > 1e-3)
        assert sure.sum() >= 0.95 * r['has'].sum()
        lo = (sure & r['hit']).sum(1)
        hi = lo + (r['has'] & ~sure).sum(1)
        assert (lo <= cor).all() and (cor <= hi).all(), (lo, cor, hi)
        # scored against the perturbed codes it would be another number
        other = score_ref.clips(score_ref.rows(ref, want_in, lengths, Q))[0]
        assert np.abs(other - ref_nll).max() > \
            FAR * 1e-5 * np.abs(ref_nll).max()


# ---- 5. the command lines ---------------------------------------------------
PARAMS = {"filter_width": 2, "sample_rate": 16000, "dilations": [1, 2, 4],
          "residual_channels": 32, "dilation_channels": 32,
          "quantization_channels": 256, "skip_channels": 32,
          "use_biases": True, "scalar_input": False,
          "initial_filter_width": 32, "residual_postproc": False}


def test_train_and_evaluate_with_the_flag(hip_lib, tmp_path, capsys):
    import evaluate
    import train
    params = str(tmp_path / 'params.json')
    json.dump(PARAMS, open(params, 'w'))
    common = ['--synthetic', '--wavenet_params', params, '--sample_size',
              '2000', '--batch_size', '2', '--num_steps', '3',
              '--checkpoint_every', '10']

    def run(name, more):
        logdir = str(tmp_path / name)
        assert train.main(common + ['--logdir', logdir] + more) == 0
        out = capsys.readouterr().out
        ev = [json.loads(l) for l in open(os.path.join(logdir,
                                                       'events.jsonl'))]
        assert [e['step'] for e in ev] == [0, 1, 2], out
        assert all(np.isfinite(e['loss']) for e in ev)
        return out, [e['loss'] for e in ev], logdir

    flag = ['--input_noise', '0.5,2']
    out_a, loss_a, log_a = run('a', flag)
    out_b, loss_b, _ = run('b', flag)
    out_c, loss_c, log_c = run('plain', [])
    out_d, loss_d, _ = run('seed', flag + ['--input_noise_seed', '7'])
    assert loss_a == loss_b                       # the floats, bit for bit
    assert loss_a != loss_c and loss_a != loss_d
    assert loss_a[0] != loss_c[0]                 # from the first step on
    assert 'probability 0.5, width 2, seed 0' in out_a
    assert 'perturbed' not in out_c
    a = torch.load(train.latest_checkpoint(log_a), map_location='cpu')
    c = torch.load(train.latest_checkpoint(log_c), map_location='cpu')
    assert a['input_noise'] == {'prob': 0.5, 'width': 2, 'seed': 0}
    assert 'input_noise' not in c
    data = str(tmp_path / 'wavs')
    os.makedirs(data)
    rng = np.random.default_rng(9)
    for i, n in enumerate((1300, 1700)):
        t = np.arange(n) / 16000.0
        x = 0.7 * np.sin(2 * np.pi * 200.0 * (i + 1) * t) \
            + 0.05 * rng.standard_normal(n)
        wavfile.write(os.path.join(data, 'u%d.wav' % i), 16000,
                      (np.clip(x, -1, 1) * 32767).astype(np.int16))
    ev = [train.latest_checkpoint(log_a), '--data_dir', data,
          '--wavenet_params', params, '--batch_size', '2']
    assert evaluate.main(ev + flag) == 0
    noisy = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert evaluate.main(ev) == 0
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert 'noisy_input' not in plain
    block = noisy.pop('noisy_input')
    assert noisy == plain                         # the clean pass is unchanged
    assert sorted(block) == ['accuracy', 'bits_per_sample', 'nll_per_sample',
                             'prob', 'width']
    assert block['prob'] == 0.5 and block['width'] == 2
    assert np.isfinite(block['nll_per_sample'])
    assert block['nll_per_sample'] != plain['nll_per_sample']
    assert abs(block['bits_per_sample'] * np.log(2.0) -
               block['nll_per_sample']) < 1e-12
