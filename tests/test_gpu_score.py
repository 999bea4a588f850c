"""Held-out scoring on the GPU (WaveNetModel.score, csrc/wn_loss.hip's
wn_xent_score, wavenet/evaluate.py): the kernel alone against float64 on the
same float32 logits, model parity with the float64 network on every kind of
model, consistency with the loss, the padding's content irrelevant, ragged
batches, launch-plan replay, parameters_swapped, and train.py --validation_dir
/ evaluate.py end to end.

Bars (each from the number formats, none from what the code gives):
  * kernel rows: 1e-5 absolute of the float64 value of the SAME float32 logits
    (|x| <= 16: one ulp of the row maximum is below 1e-6, expf / logf and the
    256-term sum add a few more); clip sums 1e-12 relative of math.fsum of the
    returned rows (a float64 sum of at most 1700 terms);
  * model rows (per_sample): 2e-4 absolute -- the project's fp32 bar on logits
    is 1e-4 and a row's NLL moves at most twice as far as its logits;
  * nll / count per clip and over the batch: 1e-5 relative of max(1, |ref|),
    the loss's own bar; counts exact;
  * correct: rows whose float64 top-two margin exceeds 1e-3 (ten times the
    logits' bar) must agree, the others may go either way; the former are at
    least 95 % of the rows.
"""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import score_ref
from util import O, ROOT, TINY, cfg_with, build_pair

sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

DIL = [1, 2, 4, 8, 16, 32, 64, 1, 2, 4]


def _bits(t):
    """Integer view for bit-for-bit comparisons (NaN included)."""
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64
                               else torch.int32)


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


# ---- 1. the kernel alone -----------------------------------------------------------
def _kernel(x, codes, lengths, Q, with_rows=True):
    from wavenet import _lib
    B, T, ld = x.shape
    dev = torch.device('cuda')
    xd = torch.as_tensor(x).to(dev).contiguous()
    qd = torch.as_tensor(codes).to(dev).contiguous()
    ln = None if lengths is None else \
        torch.as_tensor(np.asarray(lengths, np.int32)).to(dev)
    rows = torch.full((B, T), -7.0, dtype=torch.float32, device=dev) \
        if with_rows else None
    nll = torch.full((B,), -7.0, dtype=torch.float64, device=dev)
    cnt = torch.full((B,), -7, dtype=torch.int32, device=dev)
    cor = torch.full((B,), -7, dtype=torch.int32, device=dev)
    scratch = torch.empty(
        int(_lib.load().wn_xent_score_scratch_floats(B * T)),
        dtype=torch.float32, device=dev)
    _lib.call('wn_xent_score', _lib.ptr(xd), ld, _lib.ptr(qd), _lib.ptr(ln),
              _lib.ptr(rows), _lib.ptr(nll), _lib.ptr(cnt), _lib.ptr(cor),
              _lib.ptr(scratch), B, T, Q, _lib.stream())
    torch.cuda.synchronize()
    return rows, nll, cnt, cor


KSHAPES = [(3, 37, 256, 260), (3, 37, 64, 64), (2, 19, 512, 516),
           (3, 1700, 256, 256)]


@pytest.mark.parametrize('B, T, Q, ld', KSHAPES,
                         ids=['%dx%d_q%d_ld%d' % s for s in KSHAPES])
def test_kernel_against_float64_on_the_same_logits(hip_lib, B, T, Q, ld):
    rng = np.random.default_rng(B * T + Q)
    x = rng.uniform(-15.9, 15.9, (B, T, ld)).astype(np.float32)
    x[..., Q:] = 1e30                       # never read
    codes = rng.integers(0, Q, (B, T)).astype(np.int32)
    # (about a third of the targets are their row's arg-max: hits to count)
    pick = rng.random((B, T - 1)) < 0.3
    codes[:, 1:][pick] = np.argmax(x[:, :-1, :Q], -1)[pick]
    codes[0, 6], codes[0, 8] = -1, Q        # rows 5 and 7: no target
    lo, hi = 3, Q - 5
    x[0, 2, lo] = x[0, 2, hi] = 16.0        # the maximum twice ...
    codes[0, 3] = lo                        # ... target on the lower: a hit
    x[0, 10, lo] = x[0, 10, hi] = 16.0
    codes[0, 11] = hi                       # ... on the higher: not one
    x[0, 4, Q // 2] = np.nan
    for lengths in ([T, 1, 20][:B], None):
        r = score_ref.rows(x, codes, lengths, Q)
        ref_nll, ref_cnt, ref_cor = score_ref.clips(r)
        assert r['hit'][0, 2] and not r['hit'][0, 10] and not r['hit'][0, 4]
        assert not r['has'][0, 5] and not r['has'][0, 7]
        got = _kernel(x, codes, lengths, Q)
        rows = got[0].cpu().numpy().astype(np.float64)
        nll = got[1].cpu().numpy()
        assert got[2].cpu().tolist() == ref_cnt.tolist()
        assert got[3].cpu().tolist() == ref_cor.tolist()
        assert 0 < ref_cor[0] < ref_cnt[0]
        assert (rows[~r['has']] == 0.0).all()            # exact zeros
        nan = np.isnan(r['nll'])
        assert nan.sum() == 1 and np.isnan(rows[nan]).all()
        err = np.abs(rows - r['nll'])[~nan].max()
        print('%s lengths %s: worst row error %.3g (bar 1e-5)'
              % ((B, T, Q, ld), lengths, err))
        assert err <= 1e-5
        for b in range(B):
            want = math.fsum(rows[b])
            if math.isnan(want):
                assert math.isnan(nll[b]) and math.isnan(ref_nll[b])
            else:
                assert abs(nll[b] - want) <= 1e-12 * max(abs(want), 1e-300)
        # the same bits again, and without row_nll
        assert _same(got, _kernel(x, codes, lengths, Q))
        assert _same(got[1:], _kernel(x, codes, lengths, Q, False)[1:])


ROW_SHAPES = [(64, 64), (256, 256), (256, 260), (512, 516)]


@pytest.mark.parametrize('Q, ld', ROW_SHAPES,
                         ids=['q%d_ld%d' % s for s in ROW_SHAPES])
def test_scored_row_is_the_loss_kernels_row_bit_for_bit(hip_lib, Q, ld):
    """One clip of two samples: row 0 has a target, row 1 has none, so the
    loss kernel's partial 0 is (lse - ll) + 0 + 0 + 0, row 0's value exactly.
    Its bits equal row_nll[0] of wn_xent_score on the same buffers, through
    wn_xent and through wn_xent_masked (lengths = [2], 1 / denominator 0.5),
    in the Q == 256 arm and the generic one, with a padded leading dimension."""
    from wavenet import _lib
    rng = np.random.default_rng(Q + ld)
    x = rng.uniform(-15.9, 15.9, (1, 2, ld)).astype(np.float32)
    codes = np.array([[5, int(rng.integers(0, Q))]], np.int32)
    dev = torch.device('cuda')
    xd = torch.as_tensor(x).to(dev)
    qd = torch.as_tensor(codes).to(dev)
    assert _lib.load().wn_xent_partials(2) == 1
    part = torch.full((1,), -7.0, dtype=torch.float32, device=dev)
    _lib.call('wn_xent', _lib.ptr(xd), ld, _lib.ptr(qd), None, _lib.ptr(part),
              1, 2, Q, 0, _lib.stream())
    ln = torch.tensor([2], dtype=torch.int32, device=dev)
    inv_den = torch.tensor([0.5], dtype=torch.float32, device=dev)
    mpart = torch.full((1,), -7.0, dtype=torch.float32, device=dev)
    _lib.call('wn_xent_masked', _lib.ptr(xd), ld, _lib.ptr(qd), _lib.ptr(ln),
              _lib.ptr(inv_den), None, _lib.ptr(mpart), 1, 2, Q, 0,
              _lib.stream())
    torch.cuda.synchronize()
    for lengths, loss in ((None, part), ([2], mpart)):
        rows = _kernel(x, codes, lengths, Q)[0]
        print('Q %d ld %d lengths %s: loss partial %r scored row %r'
              % (Q, ld, lengths, float(loss[0]), float(rows[0, 0])))
        assert float(rows[0, 0]) > 0 and float(rows[0, 1]) == 0.0
        assert torch.equal(_bits(loss), _bits(rows[0, :1]))


# ---- 2. model parity with float64 ----------------------------------------------------
def _model(B, Q=256, biases=True, gc=None, Lc=None, R=32, S=64, dil=DIL,
           seed=0, rows=None, device=None, **extra):
    from wavenet import WaveNetModel, _lib
    kw = dict(extra)
    if gc:
        kw.update(global_condition_channels=gc, global_condition_cardinality=gc)
    net = WaveNetModel(B, dil, 2, R, R, S, quantization_channels=Q,
                       use_biases=biases, seed=seed, device=device,
                       local_condition_channels=Lc, **kw)
    g = torch.Generator().manual_seed(seed + 7)
    with torch.no_grad():
        for n, v in net.named_variables():
            last = n.split('/')[-1]
            if '/lc_upsample/' in n or '/lc_context/' in n:
                v.copy_((0.5 * torch.randn(v.shape, generator=g,
                                           dtype=torch.float64)
                         / np.sqrt(max(v.shape[0], 1))).float())
            elif 'bias' in last:
                v.copy_(0.1 * torch.randn(v.shape, generator=g,
                                          dtype=torch.float64).float())
    if rows is not None:
        net.stack_variant = _lib.stack_variant(rows=rows)
    return net


def _codes(B, T, Q, seed):
    return np.random.default_rng(seed).integers(0, Q, (B, T)).astype(np.int32)


def _assert_score(tag, s, ref_logits, codes, lengths, Q, min_sure=0.95):
    """The bars of this file's docstring; prints every figure first."""
    torch.cuda.synchronize()
    B, T = codes.shape
    r = score_ref.rows(ref_logits, codes, lengths, Q)
    ref_nll, ref_cnt, _ = score_ref.clips(r)
    nll = s.nll.cpu().numpy()
    cnt = s.count.cpu().numpy()
    cor = s.correct.cpu().numpy()
    n = np.full(B, T) if lengths is None else np.asarray(lengths)
    assert s.nll.dtype == torch.float64 and s.count.dtype == torch.int32
    assert s.correct.dtype == torch.int32
    assert cnt.tolist() == (n - 1).tolist() == ref_cnt.tolist()
    if s.per_sample is not None:
        ps = s.per_sample.cpu().numpy().astype(np.float64)
        assert ps.shape == (B, T) and s.per_sample.dtype == torch.float32
        err = np.abs(ps - r['nll']).max()
        print('%s: worst per_sample error %.3g (bar 2e-4)' % (tag, err))
        assert (ps[~r['has']] == 0.0).all()
        assert err <= 2e-4
    for b in range(B):
        if cnt[b] == 0:
            assert nll[b] == 0.0
            continue
        got, ref = nll[b] / cnt[b], ref_nll[b] / ref_cnt[b]
        print('%s: clip %d nll/count %.9g reference %.9g' % (tag, b, got, ref))
        assert abs(got - ref) <= 1e-5 * max(1.0, abs(ref))
    got, ref = nll.sum() / cnt.sum(), ref_nll.sum() / ref_cnt.sum()
    print('%s: batch nll/count %.9g reference %.9g relative error %.3g'
          % (tag, got, ref, abs(got - ref) / max(1.0, abs(ref))))
    assert abs(got - ref) <= 1e-5 * max(1.0, abs(ref))
    sure = r['has'] & (r['margin'] > 1e-3)
    frac = sure.sum() / max(r['has'].sum(), 1)
    print('%s: %.4f of the rows have a top-two margin above 1e-3; correct %s'
          % (tag, frac, cor.tolist()))
    assert frac >= min_sure
    lo = (sure & r['hit']).sum(1)
    hi = lo + (r['has'] & ~sure).sum(1)
    assert (lo <= cor).all() and (cor <= hi).all(), (lo, cor, hi)


def _assert_path(net, B, T, fwd, rows=None):
    from wavenet import _lib, train_pass
    ws = net._ws[(B, T, False)]
    assert not ws.training
    path = train_pass.step_path(net, ws, False)
    assert path.fwd.startswith(fwd), path
    if rows is not None:
        assert _lib.load().wn_stack_tile_rows(B, T, ws.stack_variant) == rows
    assert not any(w.training for w in net._ws.values())   # forward-only


# (name, model keywords, T, lengths, forward path, tile rows, float audio)
CASES = [
    ('q256_bias_rows16', dict(Q=256, biases=True, rows=16), 300,
     [300, 141, 1], 'stack', 16, False),
    ('q64_nobias_gc_rows32_audio', dict(Q=64, biases=False, gc=3, rows=32),
     330, [330, 2, 200], 'stack', 32, True),
    ('lc_rows_gc_bias', dict(Q=256, biases=True, gc=2, Lc=20), 400,
     [123, 400, 1], 'stack_lc', 32, False),
    ('blocked_r64', dict(Q=64, biases=True, R=64, S=32,
                         dil=[1, 2, 4, 8, 16, 1, 2]), 150, [150, 77],
     'blocked', None, False),
]


def _case_inputs(kw, T, lengths, audio):
    B = len(lengths)
    Q, Lc, gc = kw.get('Q', 256), kw.get('Lc'), kw.get('gc')
    rng = np.random.default_rng(T + B)
    lc = rng.standard_normal((B, T, Lc)).astype(np.float32) if Lc else None
    ids = None if gc is None else np.arange(B) % gc
    a = None
    if audio:
        a = rng.uniform(-1, 1, (B, T)).astype(np.float32)
        codes = O.mu_law_encode(a, Q)
    else:
        codes = _codes(B, T, Q, T)
    return codes, a, lc, ids


@pytest.mark.parametrize('name, kw, T, lengths, fwd, rows, audio', CASES,
                         ids=[c[0] for c in CASES])
def test_score_matches_float64(hip_lib, name, kw, T, lengths, fwd, rows,
                               audio):
    B = len(lengths)
    net = _model(B, seed=T, **kw)
    codes, a, lc, ids = _case_inputs(kw, T, lengths, audio)
    if audio:
        s = net.score(a, ids, local_condition_batch=lc, lengths=lengths,
                      per_sample=True)
    else:
        s = net.score_from_codes(torch.as_tensor(codes).cuda(), ids,
                                 local_condition_batch=lc,
                                 lengths=np.asarray(lengths), per_sample=True)
    _assert_path(net, B, T, fwd, rows)
    ref = score_ref.model_logits(net, kw.get('dil', DIL), codes, lc, ids)
    _assert_score(name, s, ref, codes, lengths, net.Q)
    # per_sample is opt-in, and asking for it changes nothing else
    s2 = net.score_from_codes(torch.as_tensor(codes).cuda(), ids,
                              local_condition_batch=lc, lengths=lengths)
    assert s2.per_sample is None and _same(s[:3], s2[:3])
    # every tensor lives on the device: nothing was fetched
    assert all(t.is_cuda for t in s)
    assert float(net.grads.abs().max()) == 0.0            # no gradient bucket


def test_score_lc_frames_with_context_and_offsets(hip_lib):
    B, T, Lc, scales, p, hop = 2, 260, 20, (2, 5), 1, 10
    lengths, offs = [260, 2], [7, 31]
    net = _model(B, Q=64, biases=False, Lc=Lc, seed=4,
                 local_condition_upsample_scales=scales,
                 local_condition_context=p)
    rng = np.random.default_rng(8)
    F = (max(offs) + T - 1) // hop + 1
    frames = rng.standard_normal((B, F, Lc)).astype(np.float32)
    codes = _codes(B, T, 64, 3)
    s = net.score_from_codes(torch.as_tensor(codes).cuda(),
                             local_condition_batch=frames,
                             local_condition_offset=offs, lengths=lengths,
                             per_sample=True)
    _assert_path(net, B, T, 'stack_lc', 32)
    ref = score_ref.model_logits(net, DIL, codes, frames=frames, offsets=offs,
                                 scales=scales)
    _assert_score('lc_frames_ctx', s, ref, codes, lengths, 64)


def test_score_scalar_input(hip_lib):
    cfg = cfg_with(TINY, batch_size=3, scalar_input=True,
                   initial_filter_width=4)
    B, T, lengths = 3, 70, [31, 70, 2]
    net, var = build_pair(cfg)
    audio = np.random.default_rng(2).uniform(-1, 1, (B, T)).astype(np.float32)
    s = net.score(audio, lengths=lengths, per_sample=True)
    _assert_path(net, B, T, 'stack')
    codes = O.mu_law_encode(audio, cfg['quantization_channels'])
    ref = score_ref.oracle_logits(cfg, var, audio)
    _assert_score('scalar_input', s, ref, codes, lengths,
                  cfg['quantization_channels'])


def test_score_generic_filter_width(hip_lib):
    """Filter width 3: the generic-tap layer kernels."""
    cfg = cfg_with(TINY, batch_size=2, filter_width=3)
    B, T, lengths = 2, 90, [90, 40]
    net, var = build_pair(cfg)
    audio = np.random.default_rng(5).uniform(-1, 1, (B, T)).astype(np.float32)
    s = net.score(audio, lengths=lengths, per_sample=True)
    _assert_path(net, B, T, 'layer_k')
    codes = O.mu_law_encode(audio, cfg['quantization_channels'])
    ref = score_ref.oracle_logits(cfg, var, audio)
    _assert_score('filter_width_3', s, ref, codes, lengths,
                  cfg['quantization_channels'])


# ---- 3. consistency with the loss ----------------------------------------------------
def test_score_tells_the_loss_story(hip_lib):
    B, T, Q = 3, 300, 256
    lengths = [300, 141, 1]
    net = _model(B, Q=Q, gc=2, seed=3)
    q = torch.as_tensor(_codes(B, T, Q, 9)).cuda()
    ids = [0, 1, 1]
    for n, den in ((lengths, sum(lengths)), (None, B * T)):
        s = net.score_from_codes(q, ids, lengths=n)
        loss = float(net.loss_from_codes(q, ids, backward=False, lengths=n))
        got = float(s.nll.sum()) / den
        print('lengths %s: nll.sum() / %d = %.9g, loss = %.9g, relative '
              'difference %.3g' % (n, den, got, loss, abs(got - loss) / loss))
        assert abs(got - loss) <= 1e-6 * abs(loss)


# ---- 4. padding ----------------------------------------------------------------------
def test_padding_content_is_irrelevant(hip_lib):
    B, T, Q, Lc = 3, 400, 256, 12
    lengths = [400, 123, 1]
    net = _model(B, Q=Q, gc=3, Lc=Lc, seed=2)
    rng = np.random.default_rng(5)
    codes = _codes(B, T, Q, 6)
    lc = rng.standard_normal((B, T, Lc)).astype(np.float32)
    res = []
    for fill_codes, fill_lc in ((False, False), (True, False), (True, True)):
        c, r = codes.copy(), lc.copy()
        for b, n in enumerate(lengths):
            c[b, n:] = rng.integers(0, Q, T - n) if fill_codes else 0
            r[b, n:] = rng.standard_normal(r[b, n:].shape) if fill_lc else 0
        res.append(net.score_from_codes(
            torch.as_tensor(c).cuda(), [0, 1, 2], local_condition_batch=r,
            lengths=lengths, per_sample=True))
    torch.cuda.synchronize()
    assert float(res[0].nll[0]) > 0
    for s in res[1:]:
        assert _same(s, res[0])
    for b, n in enumerate(lengths):
        assert int(torch.count_nonzero(res[0].per_sample[b, n - 1:])) == 0
        assert n < 2 or float(res[0].per_sample[b, :n - 1].min()) > 0
    # without lengths the padding does matter (the test can see it)
    a = net.score_from_codes(torch.as_tensor(codes).cuda(), [0, 1, 2],
                             local_condition_batch=lc)
    assert not torch.equal(a.nll, res[0].nll)


def test_padding_frames_are_irrelevant(hip_lib):
    B, T, Lc, scales, p, hop = 2, 300, 10, (4, 5), 1, 20
    lengths, offs = [300, 90], [25, 3]
    net = _model(B, Q=64, Lc=Lc, seed=6,
                 local_condition_upsample_scales=scales,
                 local_condition_context=p)
    rng = np.random.default_rng(3)
    F = (max(offs) + T - 1) // hop + 1
    frames = rng.standard_normal((B, F, Lc)).astype(np.float32)
    last = (offs[1] + lengths[1] - 1) // hop + p
    assert last + 1 < F
    f0 = frames.copy()
    f0[1, last + 1:] = 0
    q = torch.as_tensor(_codes(B, T, 64, 7)).cuda()
    res = [net.score_from_codes(q, local_condition_batch=f,
                                local_condition_offset=offs, lengths=lengths,
                                per_sample=True) for f in (f0, frames)]
    assert _same(res[0], res[1]) and float(res[0].nll[1]) > 0


# ---- 5. ragged batches ---------------------------------------------------------------
def test_ragged_batches(hip_lib):
    T, Q = 260, 256
    net = _model(3, Q=Q, gc=2, seed=5)
    for B, lengths in ((2, [260, 77]), (5, [260, 1, 2, 133, 260])):
        codes = _codes(B, T, Q, B)
        ids = np.arange(B) % 2
        s = net.score_from_codes(torch.as_tensor(codes).cuda(), ids,
                                 lengths=lengths, per_sample=True)
        assert s.nll.shape == (B,) and s.per_sample.shape == (B, T)
        ref = score_ref.model_logits(net, DIL, codes, gc_ids=ids)
        _assert_score('ragged B = %d' % B, s, ref, codes, lengths, Q)
    # float audio in, and the model's own batch size from a flat input
    audio = np.random.default_rng(1).uniform(-1, 1, (5, T)).astype(np.float32)
    s = net.score(audio, np.arange(5) % 2)
    assert s.nll.shape == (5,) and s.count.cpu().tolist() == [T - 1] * 5
    s = net.score(audio[:3].reshape(-1), [0, 1, 0])
    assert s.nll.shape == (3,)


# ---- 6. launch-plan replay -----------------------------------------------------------
def test_replay_sees_new_lengths_and_codes(hip_lib):
    B, T, Q = 3, 300, 256
    net = _model(B, Q=Q, gc=2, seed=5)
    assert net.use_launch_plans
    ids = [1, 0, 1]
    ws = None
    for i, lengths in enumerate(([300, 141, 1], [17, 300, 299], None,
                                 [1, 1, 300])):
        codes = _codes(B, T, Q, 40 + i)
        s = net.score_from_codes(torch.as_tensor(codes).cuda(), ids,
                                 lengths=lengths, per_sample=True)
        torch.cuda.synchronize()
        assert ws is None or ws is net._ws[(B, T, False)]
        ws = net._ws[(B, T, False)]
        ref = score_ref.model_logits(net, DIL, codes, gc_ids=ids)
        _assert_score('call %d' % i, s, ref, codes, lengths, Q)
    assert any(isinstance(p, list) for p in ws.plans.values())   # recorded


# ---- 7. parameters_swapped -----------------------------------------------------------
def test_parameters_swapped(hip_lib):
    from wavenet import evaluate as ev
    B, T, Q = 2, 300, 256
    lengths = [300, 120]
    net = _model(B, Q=Q, gc=2, seed=1)
    other = _model(B, Q=Q, gc=2, seed=1)
    q = torch.as_tensor(_codes(B, T, Q, 2)).cuda()
    ids = [0, 1]

    def run(m):
        # (twice: the second call replays or records a launch plan)
        m.score_from_codes(q, ids, lengths=lengths)
        s = m.score_from_codes(q, ids, lengths=lengths, per_sample=True)
        return [t.clone() for t in s]
    before = run(net)
    loss_before = net.loss_from_codes(q, ids, backward=False,
                                      lengths=lengths).clone()
    g = torch.Generator().manual_seed(3)
    flat = (net.params.cpu() * (1 + 0.05 * torch.randn(
        net.params.numel(), generator=g))).cuda()
    with torch.no_grad():
        other.params.copy_(flat)
    want = run(other)
    with ev.parameters_swapped(net, flat):
        inside = run(net)
    assert _same(inside, want) and not _same(inside, before)
    assert _same(run(net), before)
    assert torch.equal(net.loss_from_codes(q, ids, backward=False,
                                           lengths=lengths), loss_before)


# ---- 8. end to end -------------------------------------------------------------------
SMALL = {"filter_width": 2, "sample_rate": 16000,
         "dilations": [1, 2, 4, 8, 16, 32, 1, 2, 4, 8, 16, 32],
         "residual_channels": 32, "dilation_channels": 32,
         "quantization_channels": 256, "skip_channels": 64,
         "use_biases": True, "scalar_input": False,
         "initial_filter_width": 32, "residual_postproc": False}


def test_train_validates_and_evaluate_cli_agrees(hip_lib, tmp_path, capsys):
    import evaluate
    import generate
    import train
    from wavenet import WaveNetModel
    from wavenet import evaluate as ev
    params = str(tmp_path / 'params.json')
    json.dump(SMALL, open(params, 'w'))
    data = str(tmp_path / 'held_out')
    os.makedirs(data)
    for i, n in enumerate([3000, 1700, 2400]):
        t = np.arange(n) / 16000.0
        a = 0.5 * np.sin(2 * np.pi * (220 + 60 * i) * t + 0.3)
        wavfile.write(os.path.join(data, 'clip%d.wav' % i), 16000,
                      (a * 32767).astype(np.int16))
    logdir = str(tmp_path / 'log')
    common = ['--wavenet_params', params, '--sample_size', '2000',
              '--batch_size', '2', '--silence_threshold', '0']
    assert train.main(['--synthetic', '--logdir', logdir, '--num_steps', '4',
                       '--validate_every', '2', '--validation_dir', data,
                       '--learning_rate', '0.002', '--ema_decay', '0.5']
                      + common) == 0
    out = capsys.readouterr().out
    ev_lines = [json.loads(l) for l in open(os.path.join(logdir,
                                                         'events.jsonl'))]
    val = [e for e in ev_lines if 'validation_loss' in e]
    assert [e['step'] for e in val] == [0, 2, 3]      # every 2, and the last
    for e in val:
        assert sorted(e) == ['step', 'validation_accuracy', 'validation_bits',
                             'validation_loss', 'validation_samples']
        assert all(np.isfinite(e[k]) for k in e)
        assert abs(e['validation_bits'] * math.log(2.0)
                   - e['validation_loss']) < 1e-9
        assert e['validation_samples'] > 0 and 0 <= e['validation_accuracy'] <= 1
        assert 'step %d - validation loss = %.3f, bits/sample = %.3f, ' \
            'accuracy = %.3f' % (e['step'], e['validation_loss'],
                                 e['validation_bits'],
                                 e['validation_accuracy']) in out
    # the lines stay in order: step k's training line, then its validation
    order = [(e['step'], 'validation_loss' in e) for e in ev_lines]
    assert order == sorted(order)
    assert [e['step'] for e in ev_lines if 'loss' in e] == [0, 1, 2, 3]
    ckpt = train.latest_checkpoint(logdir)
    assert ckpt.endswith('model.ckpt-3')
    for use_ema in (False, True):
        flags = ['--use_ema', 'true'] if use_ema else []
        assert evaluate.main([ckpt, '--data_dir', data] + common + flags) == 0
        line = capsys.readouterr().out.strip().splitlines()[-1]
        got = json.loads(line)
        assert sorted(got) == ['accuracy', 'bits_per_sample', 'clips',
                               'nll_per_sample', 'samples']
        net = WaveNetModel(2, SMALL['dilations'], 2, 32, 32, 64,
                           quantization_channels=256, use_biases=True)
        assert generate.restore(net, ckpt, use_ema) is None
        capsys.readouterr()
        data_set = ev.ValidationSet(data, 16000, sample_size=2000,
                                    silence_threshold=0.0)
        want = ev.evaluate(net, data_set.batches(2))
        assert got['nll_per_sample'] == want['nll_per_sample']
        assert got == want and got['clips'] == len(data_set)
        if not use_ema:
            # the weights after the last step: train.py's last validation
            assert abs(val[-1]['validation_loss'] - got['nll_per_sample']) \
                <= 1e-9 * got['nll_per_sample']
            raw = got
    assert got['nll_per_sample'] != raw['nll_per_sample']      # EMA differs
