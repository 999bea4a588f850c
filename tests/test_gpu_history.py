"""Piece history on the GPU (`history` on WaveNetModel.loss / score,
csrc/wn_loss.hip's xent_window_kernel and the scoring kernels' starts;
DeviceCorpus(history=), csrc/wn_corpus.hip's _hist entries): parity with the
float64 restatement (tests/hist_ref.py), history = 0 bitwise today's call,
the silence of the history rows, the score, the point of the feature -- a
piece behind its receptive field scores like its place in the utterance --
the gathers, and the command lines.

Bars: those of tests/test_gpu_masked_loss.py for the loss (1e-5 relative)
and the gradients (TOL = 2e-5 of each variable's largest entry); those of
tests/test_gpu_score.py for the score (per_sample 2e-4, nll / count 1e-5
relative, hits counted exactly where the float64 top-two margin exceeds
1e-3); 1e-5 per row for a piece against its utterance."""
import json
import math
import os
import re
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import corpus_ref as R
import hist_ref
import lc_ref
import score_ref
from util import ROOT

sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

TOL = 2e-5
DIL = [1, 2, 4, 8, 1, 2, 4, 8]        # receptive field 32
B, T = 3, 100
LENGTHS = [100, 71, 40]
HIST = [0, 7, 32]


def _model(B, Q=256, biases=True, gc=None, Lc=None, R=32, S=64, dil=DIL,
           seed=0, fw=2, **extra):
    from wavenet import WaveNetModel
    kw = dict(extra)
    if gc:
        kw.update(global_condition_channels=gc, global_condition_cardinality=gc)
    net = WaveNetModel(B, dil, fw, R, R, S, quantization_channels=Q,
                       use_biases=biases, seed=seed,
                       local_condition_channels=Lc, **kw)
    g = torch.Generator().manual_seed(seed + 7)
    with torch.no_grad():
        for n, v in net.named_variables():
            last = n.split('/')[-1]
            if '/lc_upsample/' in n:
                v.copy_((0.5 * torch.randn(v.shape, generator=g,
                                           dtype=torch.float64)
                         / np.sqrt(max(v.shape[0], 1))).float())
            elif 'bias' in last:
                v.copy_(0.1 * torch.randn(v.shape, generator=g,
                                          dtype=torch.float64).float())
    return net


def _codes(B, T, Q, seed):
    return np.random.default_rng(seed).integers(0, Q, (B, T)).astype(np.int32)


def _bh(history, n):
    return np.broadcast_to(np.asarray(history), (len(n),))


def _assert_close(tag, loss, grads, ref_loss, ref_g):
    got, ref = dict(lc_ref.flatten(grads)), dict(lc_ref.flatten(ref_g))
    assert sorted(got) == sorted(ref)
    print('%s: loss %.9g reference %.9g relative error %.3g'
          % (tag, loss, ref_loss, abs(loss - ref_loss) / max(1.0, abs(ref_loss))))
    worst = (0.0, None)
    for k in sorted(ref):
        scale = max(np.abs(ref[k]).max(), 1e-30)
        worst = max(worst, (np.abs(got[k] - ref[k]).max() / scale, k))
    print('%s: worst gradient error %.3g of the largest entry (%s), bar %g'
          % (tag, worst[0], worst[1], TOL))
    assert abs(loss - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), \
        (loss, ref_loss)
    assert max(np.abs(a).max() for a in ref.values()) > 0
    for k in sorted(ref):
        scale = np.abs(ref[k]).max()
        err = np.abs(got[k] - ref[k]).max()
        assert err <= TOL * max(scale, 1e-30), (tag, k, err, scale)


def _bucket(net):
    torch.cuda.synchronize()
    return net.grads.clone()


def _assert_silent(dl, lengths, history):
    """dlogits [B, T, Q]: exact zeros on the history rows t + 1 < h and on
    the padding, something on the rows between."""
    for b, (n, h) in enumerate(zip(lengths, _bh(history, lengths))):
        first = max(int(h) - 1, 0)
        assert int(torch.count_nonzero(dl[b, :first])) == 0, b
        assert int(torch.count_nonzero(dl[b, n:])) == 0, b
        assert bool((dl[b, first:n].abs().max(-1).values > 0).all()), b


# ---- 6. loss and gradients against float64 -------------------------------------
SCALES, HOP, OFFS = (4, 5), 20, [7, 131, 45]
CASES = [
    ('q256_bias', dict(Q=256, biases=True)),
    ('q64_nobias_gc', dict(Q=64, biases=False, gc=3)),
    ('q256_lc_rows_gc', dict(Q=256, biases=True, gc=2, Lc=20)),
    ('q64_lc_rows_nobias', dict(Q=64, biases=False, Lc=12)),
    ('q64_upsampler_offsets', dict(Q=64, biases=False, gc=3, Lc=10,
                                   local_condition_upsample_scales=SCALES)),
    ('q256_upsampler_offsets', dict(Q=256, biases=False, Lc=10,
                                    local_condition_upsample_scales=SCALES)),
    ('q64_blocked_r64', dict(Q=64, biases=True, R=64, S=32)),
]


@pytest.mark.parametrize('history', [HIST, 5], ids=['h_0_7_32', 'h_5'])
@pytest.mark.parametrize('name, kw', CASES, ids=[c[0] for c in CASES])
def test_loss_and_gradients_match_float64(hip_lib, name, kw, history):
    net = _model(B, seed=11, **kw)
    Q, Lc, gc = net.Q, kw.get('Lc'), kw.get('gc')
    up = 'local_condition_upsample_scales' in kw
    rng = np.random.default_rng(len(name))
    ids = None if gc is None else np.arange(B) % gc
    codes = _codes(B, T, Q, 3)
    lc = offs = frames = None
    call = dict(lengths=LENGTHS, history=history)
    if up:
        F = (max(OFFS) + T - 1) // HOP + 1
        frames = rng.standard_normal((B, F, Lc)).astype(np.float32)
        offs = OFFS
        call.update(local_condition_batch=frames, local_condition_offset=offs)
    elif Lc:
        lc = rng.standard_normal((B, T, Lc)).astype(np.float32)
        call.update(local_condition_batch=lc)
    q = torch.as_tensor(codes).cuda()
    loss = float(net.loss_from_codes(q, ids, **call))
    torch.cuda.synchronize()
    assert net.blocked == (kw.get('R', 32) > 32)
    ref_loss, ref_g = hist_ref.loss_and_grads(
        lc_ref.model_tree(net), DIL, codes, LENGTHS, history, lc, gc_ids=ids,
        frames=frames, offsets=offs, scales=SCALES if up else None,
        use_biases=net.use_biases, quantization_channels=Q,
        relu_masks=lc_ref.device_relu_masks(net, B, T))
    _assert_close(name, loss, lc_ref.model_tree(net, grads=True), ref_loss,
                  ref_g)
    # the backward GEMMs read dlogits in place: still in the logits buffer
    _assert_silent(net._ws[(B, T, True)].logits.reshape(B, T, Q), LENGTHS,
                   history)
    # forward only: the same loss, nothing else
    fwd = float(net.loss_from_codes(q, ids, backward=False, **call))
    assert abs(fwd - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))


def test_history_without_lengths_and_denominator(hip_lib):
    """Without lengths n[b] = T; loss_denominator still overrides."""
    net = _model(B, Q=256, seed=5)
    codes = _codes(B, T, 256, 8)
    q = torch.as_tensor(codes).cuda()
    h = [0, 99, 100]                      # (a clip without any target)
    loss = float(net.loss_from_codes(q, history=h))
    torch.cuda.synchronize()
    ref_loss, ref_g = hist_ref.loss_and_grads(
        lc_ref.model_tree(net), DIL, codes, None, h, use_biases=True,
        relu_masks=lc_ref.device_relu_masks(net, B, T))
    _assert_close('no lengths', loss, lc_ref.model_tree(net, grads=True),
                  ref_loss, ref_g)
    a = net.loss_from_codes(q, history=h, lengths=[T] * B).clone()
    ga = _bucket(net)
    assert float(a) == loss
    d = hist_ref.denominator([T] * B, h)
    same = net.loss_from_codes(q, history=h, lengths=[T] * B,
                               loss_denominator=d).clone()
    assert torch.equal(a, same) and torch.equal(ga, _bucket(net))
    half = net.loss_from_codes(q, history=h, lengths=[T] * B,
                               loss_denominator=2 * d).clone()
    assert torch.equal(half * 2, a) and torch.equal(_bucket(net) * 2, ga)


# ---- 7. history = 0 is today's call -------------------------------------------
def _same_score(a, b):
    return all((x is None and y is None) or torch.equal(x, y)
               for x, y in zip(a, b))


@pytest.mark.parametrize('Q', [256, 64])
def test_history_zero_is_todays_call_bit_for_bit(hip_lib, Q):
    net = _model(B, Q=Q, gc=2, Lc=16, seed=1)
    assert net.use_launch_plans
    q = torch.as_tensor(_codes(B, T, Q, 1)).cuda()
    lc = np.random.default_rng(1).standard_normal((B, T, 16)).astype(np.float32)
    ids = [0, 1, 0]
    for lengths in (None, LENGTHS):
        kw = dict(local_condition_batch=lc)
        if lengths is not None:
            kw['lengths'] = lengths
        for _ in range(3):              # eager, recorded, replayed
            a = net.loss_from_codes(q, ids, **kw).clone()
            ga = _bucket(net)
            assert float(ga.abs().max()) > 0
            # the staged history changes between the replays
            c = net.loss_from_codes(q, ids, history=HIST, **kw).clone()
            assert not torch.equal(a, c) and not torch.equal(ga, _bucket(net))
            for zero in (0, [0, 0, 0], np.zeros(B, np.int64)):
                b = net.loss_from_codes(q, ids, history=zero, **kw).clone()
                assert torch.equal(a, b), (float(a), float(b))
                assert torch.equal(ga, _bucket(net))
        ws = net._ws[(B, T, True)]
        assert any(isinstance(p, list) for p in ws.plans.values())  # recorded
        f0 = net.loss_from_codes(q, ids, backward=False, **kw).clone()
        net.loss_from_codes(q, ids, backward=False, history=HIST, **kw)
        f1 = net.loss_from_codes(q, ids, backward=False, history=0, **kw)
        assert torch.equal(f0, f1)
        for _ in range(2):
            s0 = net.score_from_codes(q, ids, per_sample=True, **kw)
            s0 = [t.clone() for t in s0]
            moved = net.score_from_codes(q, ids, per_sample=True, history=HIST,
                                         **kw)
            assert not torch.equal(moved.nll, s0[0])
            s1 = net.score_from_codes(q, ids, per_sample=True, history=0, **kw)
            assert _same_score(s0, s1)
            assert float(s1.per_sample.abs().max()) > 0


# ---- 8. history rows are silent; the kernels on planted logits -----------------
def _window_kernels(x, codes, lengths, history, Q, quirk=1):
    """wn_xent_window and wn_xent_score_window on given logits [B, T, ld]:
    (loss sum, dlogits [B, T, ld], row_nll, clip_nll, count, correct)."""
    from wavenet import _lib
    dev = torch.device('cuda')
    Bn, Tn, ld = x.shape
    xd = torch.as_tensor(x).to(dev).contiguous()
    qd = torch.as_tensor(codes.astype(np.int32)).to(dev)
    ln = torch.as_tensor(np.asarray(lengths, np.int32)).to(dev)
    hs = torch.as_tensor(np.asarray(history, np.int32)).to(dev)
    den = float((np.asarray(lengths) - np.asarray(history)).sum())
    inv = torch.tensor([1.0 / den], dtype=torch.float32, device=dev)
    dl = torch.full((Bn, Tn, ld), -7.0, dtype=torch.float32, device=dev)
    nparts = _lib.load().wn_xent_partials(Bn * Tn)
    parts = torch.full((nparts,), -7.0, dtype=torch.float32, device=dev)
    _lib.call('wn_xent_window', _lib.ptr(xd), ld, _lib.ptr(qd), _lib.ptr(hs),
              _lib.ptr(ln), _lib.ptr(inv), _lib.ptr(dl), _lib.ptr(parts), Bn,
              Tn, Q, quirk, _lib.stream())
    rows = torch.full((Bn, Tn), -7.0, dtype=torch.float32, device=dev)
    nll = torch.full((Bn,), -7.0, dtype=torch.float64, device=dev)
    cnt = torch.full((Bn,), -7, dtype=torch.int32, device=dev)
    cor = torch.full((Bn,), -7, dtype=torch.int32, device=dev)
    scratch = torch.empty(
        int(_lib.load().wn_xent_score_scratch_floats(Bn * Tn)),
        dtype=torch.float32, device=dev)
    _lib.call('wn_xent_score_window', _lib.ptr(xd), ld, _lib.ptr(qd),
              _lib.ptr(hs), _lib.ptr(ln), _lib.ptr(rows), _lib.ptr(nll),
              _lib.ptr(cnt), _lib.ptr(cor), _lib.ptr(scratch), Bn, Tn, Q,
              _lib.stream())
    torch.cuda.synchronize()
    return parts.double().sum().item(), dl, rows, nll, cnt, cor


# (Q, ld): the single-pass row path and the generic one, a padded leading
# dimension; T = 100 rows per clip: 75 workgroups of four rows
KSHAPES = [(256, 256), (256, 260), (64, 64), (512, 516)]


@pytest.mark.parametrize('Q, ld', KSHAPES, ids=['q%d_ld%d' % s for s in KSHAPES])
def test_kernels_ignore_what_the_history_rows_hold(hip_lib, Q, ld):
    rng = np.random.default_rng(Q + ld)
    x = rng.uniform(-15.9, 15.9, (B, T, ld)).astype(np.float32)
    x[..., Q:] = 1e30                       # never read
    codes = rng.integers(0, Q, (B, T)).astype(np.int32)
    pick = rng.random((B, T - 1)) < 0.3     # hits to count
    codes[:, 1:][pick] = np.argmax(x[:, :-1, :Q], -1)[pick]
    lengths = LENGTHS
    for history in ([0, 7, 32], [5, 5, 5], [100, 1, 40], [0, 0, 0]):
        r = hist_ref.rows(x, codes, lengths, history, Q)
        ref_nll, ref_cnt, ref_cor = hist_ref.clips(r)
        assert ref_cnt.tolist() == [n - max(h, 1)
                                    for n, h in zip(lengths, history)]
        clean = _window_kernels(x, codes, lengths, history, Q)
        # NaN in every row without a target but the label-less last row (which
        # the quirk evaluates), other codes where only such a row looks
        planted, c2 = x.copy(), codes.copy()
        for b, (n, h) in enumerate(zip(lengths, history)):
            planted[b, :max(h - 1, 0), :Q] = np.nan
            planted[b, n:, :Q] = np.nan
            c2[b, 1:h] = (c2[b, 1:h] + 1 + b) % Q
            c2[b, n:] = -5
        got = _window_kernels(planted, c2, lengths, history, Q)
        for a, b_ in zip(clean, got):
            if isinstance(a, float):
                assert a == b_ and math.isfinite(a)
            else:
                assert torch.equal(a, b_)
        loss_sum, dl, rows, nll, cnt, cor = got
        assert bool(torch.isfinite(dl[..., :Q]).all())
        assert bool((dl[..., Q:] == -7.0).all())          # never written
        _assert_silent(dl[..., :Q], lengths, history)
        assert bool(torch.isfinite(rows).all()) and \
            bool(torch.isfinite(nll).all())
        rows = rows.cpu().numpy().astype(np.float64)
        assert (rows[~r['has']] == 0.0).all()
        err = np.abs(rows - r['nll']).max()
        print('Q %d ld %d history %s: worst row error %.3g (bar 1e-5)'
              % (Q, ld, history, err))
        assert err <= 1e-5
        assert cnt.cpu().tolist() == ref_cnt.tolist()
        assert cor.cpu().tolist() == ref_cor.tolist()
        nll = nll.cpu().numpy()
        for b in range(B):
            want = math.fsum(rows[b])
            assert abs(nll[b] - want) <= 1e-12 * max(abs(want), 1e-300)
        # the loss kernel sums the same rows (float32 partials)
        assert abs(loss_sum - rows.sum()) <= 1e-5 * max(1.0, rows.sum())
    # starts all zero: wn_xent_masked's and wn_xent_score's bits
    from wavenet import _lib
    dev = torch.device('cuda')
    xd, qd = torch.as_tensor(x).to(dev), torch.as_tensor(codes).to(dev)
    ln = torch.as_tensor(np.asarray(lengths, np.int32)).to(dev)
    inv = torch.tensor([1.0 / sum(lengths)], dtype=torch.float32, device=dev)
    dl = torch.full((B, T, ld), -7.0, dtype=torch.float32, device=dev)
    parts = torch.full((_lib.load().wn_xent_partials(B * T),), -7.0,
                       dtype=torch.float32, device=dev)
    _lib.call('wn_xent_masked', _lib.ptr(xd), ld, _lib.ptr(qd), _lib.ptr(ln),
              _lib.ptr(inv), _lib.ptr(dl), _lib.ptr(parts), B, T, Q, 1,
              _lib.stream())
    torch.cuda.synchronize()
    assert torch.equal(dl, clean[1])
    assert parts.double().sum().item() == clean[0]


def test_history_rows_of_a_backward_pass_are_zero(hip_lib):
    """Through the model, with and without lengths, one int for all clips."""
    for Q in (256, 64):
        net = _model(B, Q=Q, seed=2)
        q = torch.as_tensor(_codes(B, T, Q, 5)).cuda()
        for lengths, history in ((LENGTHS, HIST), (None, 33), (LENGTHS, 40),
                                 (None, [0, 1, 100])):
            kw = {} if lengths is None else dict(lengths=lengths)
            loss = net.loss_from_codes(q, history=history, **kw)
            assert math.isfinite(float(loss))
            _assert_silent(net._ws[(B, T, True)].logits.reshape(B, T, Q),
                           lengths or [T] * B, history)


# ---- 9. score ------------------------------------------------------------------
def _assert_score(tag, s, ref_logits, codes, lengths, history, Q):
    torch.cuda.synchronize()
    Bn, Tn = codes.shape
    r = hist_ref.rows(ref_logits, codes, lengths, history, Q)
    ref_nll, ref_cnt, _ = hist_ref.clips(r)
    nll, cnt = s.nll.cpu().numpy(), s.count.cpu().numpy()
    cor = s.correct.cpu().numpy()
    n = np.full(Bn, Tn) if lengths is None else np.asarray(lengths)
    assert s.nll.dtype == torch.float64 and s.count.dtype == torch.int32
    assert cnt.tolist() == ref_cnt.tolist() == \
        (n - np.maximum(_bh(history, n), 1)).tolist()
    ps = s.per_sample.cpu().numpy().astype(np.float64)
    err = np.abs(ps - r['nll']).max()
    print('%s: worst per_sample error %.3g (bar 2e-4)' % (tag, err))
    assert (ps[~r['has']] == 0.0).all() and (ps[r['has']] > 0).all()
    assert err <= 2e-4
    for b in range(Bn):
        if cnt[b] == 0:
            assert nll[b] == 0.0
            continue
        got, ref = nll[b] / cnt[b], ref_nll[b] / ref_cnt[b]
        print('%s: clip %d nll/count %.9g reference %.9g' % (tag, b, got, ref))
        assert abs(got - ref) <= 1e-5 * max(1.0, abs(ref))
    sure = r['has'] & (r['margin'] > 1e-3)
    lo = (sure & r['hit']).sum(1)
    hi = lo + (r['has'] & ~sure).sum(1)
    assert sure.sum() >= 0.95 * r['has'].sum()
    assert (lo <= cor).all() and (cor <= hi).all(), (lo, cor, hi)


@pytest.mark.parametrize('Q', [256, 64])
def test_score_matches_float64(hip_lib, Q):
    net = _model(B, Q=Q, gc=2, Lc=8, seed=3)
    codes = _codes(B, T, Q, 6)
    q = torch.as_tensor(codes).cuda()
    lc = np.random.default_rng(2).standard_normal((B, T, 8)).astype(np.float32)
    ids = np.array([1, 0, 1])
    ref = score_ref.model_logits(net, DIL, codes, lc, ids)
    for lengths, history in ((LENGTHS, HIST), (LENGTHS, 5), (None, [0, 1, 100]),
                             (LENGTHS, [100, 71, 39])):
        kw = {} if lengths is None else dict(lengths=lengths)
        s = net.score_from_codes(q, ids, local_condition_batch=lc,
                                 per_sample=True, history=history, **kw)
        _assert_score('Q %d history %s' % (Q, history), s, ref, codes,
                      lengths, history, Q)
        n = np.asarray(lengths or [T] * B)
        loss = float(net.loss_from_codes(q, ids, local_condition_batch=lc,
                                         backward=False, history=history,
                                         **kw))
        want = float(s.nll.sum()) / hist_ref.denominator(n, history)
        print('loss %.9g nll.sum() / sum(n - h) %.9g' % (loss, want))
        assert abs(loss - want) <= 1e-5 * max(1.0, abs(want))
    # float audio through score(): the same rule
    a = np.random.default_rng(4).uniform(-1, 1, (B, T)).astype(np.float32)
    s = net.score(a, ids, local_condition_batch=lc, lengths=LENGTHS,
                  history=HIST)
    assert s.per_sample is None
    assert s.count.cpu().tolist() == [99, 64, 8]


# ---- 10. the point of the feature ------------------------------------------------
@pytest.mark.parametrize('name, kw, dil', [
    ('k2_r32_q256', dict(Q=256), DIL),
    ('k3_r25_q64_generic', dict(Q=64, fw=3), [1, 2, 4])],
    ids=['k2_r32_q256', 'k3_r25_q64_generic'])
def test_a_piece_behind_its_receptive_field_scores_like_the_utterance(
        hip_lib, name, kw, dil):
    N, size = 300, 64
    net = _model(1, seed=9, dil=dil, **kw)
    Rf = net.receptive_field
    assert Rf == (32 if kw.get('fw', 2) == 2 else 25)
    assert net.generic_layers == (kw.get('fw', 2) != 2)
    codes = _codes(1, N, net.Q, 12)
    whole = net.score_from_codes(torch.as_tensor(codes).cuda(),
                                 per_sample=True)
    u_rows = whole.per_sample.cpu().numpy().astype(np.float64)[0]
    u_nll, u_cnt = float(whole.nll[0]), int(whole.count[0])
    assert u_cnt == N - 1

    def pieces(H):
        cut = hist_ref.validation_pieces(N, size, H)
        Tp = max(hi - lo for lo, hi, _ in cut)
        q = np.zeros((len(cut), Tp), np.int32)
        for j, (lo, hi, _) in enumerate(cut):
            q[j, :hi - lo] = codes[0, lo:hi]
        s = net.score_from_codes(
            torch.as_tensor(q).cuda(), per_sample=True,
            lengths=[hi - lo for lo, hi, _ in cut],
            history=[h for _, _, h in cut])
        return cut, s, s.per_sample.cpu().numpy().astype(np.float64)

    cut, s, rows = pieces(Rf)
    assert [h for _, _, h in cut] == [0] + [Rf] * 4
    worst, covered = 0.0, np.zeros(N, bool)
    for j, (lo, hi, h) in enumerate(cut):
        for t in range(max(h - 1, 0), hi - lo - 1):      # the counted rows
            worst = max(worst, abs(rows[j, t] - u_rows[lo + t]))
            assert not covered[lo + t]
            covered[lo + t] = True
    print('%s: worst counted row against the utterance %.3g (bar 1e-5)'
          % (name, worst))
    assert covered[:N - 1].all() and not covered[N - 1]
    assert worst <= 1e-5
    count = int(s.count.sum())
    total = float(s.nll.sum())
    print('%s: pieces nll %.9g utterance %.9g, %d rows' % (name, total, u_nll,
                                                         count))
    assert count == u_cnt
    assert abs(total - u_nll) <= 1e-5 * count
    # without history a piece's leading rows see zeros in front of them
    cut0, s0, rows0 = pieces(0)
    lead = max(abs(rows0[j, t] - u_rows[lo + t])
               for j, (lo, hi, _) in enumerate(cut0) if lo > 0
               for t in range(min(Rf - 1, hi - lo - 1)))
    print('%s: without history the leading rows differ by up to %.3g'
          % (name, lead))
    assert lead > 1e-5
    # ... and only those: behind the receptive field the rows agree again
    for j, (lo, hi, _) in enumerate(cut0):
        for t in range(Rf - 1, hi - lo - 1):
            assert abs(rows0[j, t] - u_rows[lo + t]) <= 1e-5


# ---- 11. gather ------------------------------------------------------------------
ULEN = [1, 2, 5, 31, 64, 65, 203, 150]
IDS = [2, 0, 1, 3, 1, 0, 2, 3]
SEED = 11
GHOP, GLC = 4, 5


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(got, want):
    return tuple(got.shape) == tuple(want.shape) and \
        np.array_equal(_bits(got), _bits(want))


def _corpus_inputs():
    rng = np.random.default_rng(0)
    utts = [rng.uniform(-1, 1, n).astype(np.float32) for n in ULEN]
    frames = [rng.standard_normal((-(-n // GHOP), GLC)).astype(np.float32)
              for n in ULEN]
    return utts, frames


@pytest.mark.parametrize('crop, size', [('pieces', 64), ('pieces', 50),
                                        ('random', 17)])
def test_gather_with_history_equals_restatement(hip_lib, crop, size):
    from wavenet.corpus import DeviceCorpus
    utts, frames = _corpus_inputs()
    kw = dict(frames=frames, hop=GHOP, sample_size=size, crop=crop, seed=SEED)
    plain = DeviceCorpus.from_arrays(utts, IDS, **kw)
    seen = set()
    for H in (0, 5, 40, 10 ** 6):
        corpus = DeviceCorpus.from_arrays(utts, IDS, history=H, **kw)
        for Bn, Tcut in ((1, None), (3, None), (5, None), (5, 20)):
            for step in range(5):
                slots, hist, Tn, orig = hist_ref.plan(
                    ULEN, size, crop, SEED, step, Bn, H, IDS, T=Tcut)
                audio = R.gather(utts, slots, Tn)
                win, offs = R.frame_windows(frames, slots, Tn, GHOP)
                rows = R.frame_rows(frames, slots, Tn, GHOP)
                for lc in ('frames', 'rows'):
                    b = corpus.batch(step, Bn, T=Tcut, lc=lc)
                    assert tuple(b.audio.shape) == (Bn, Tn)
                    assert _same_bits(b.audio, audio), (H, Bn, step)
                    assert b.lengths.tolist() == [s[2] for s in slots]
                    assert b.history.tolist() == hist
                    assert b.history.dtype == np.int64
                    assert b.gc.tolist() == [s[3] for s in slots]
                    if lc == 'frames':
                        assert _same_bits(b.frames, win), (H, Bn, step)
                        assert b.offsets.tolist() == offs.tolist()
                    else:
                        assert _same_bits(b.rows, rows), (H, Bn, step)
                    if H > 0:           # the device's copy of the plan
                        dh, dn = corpus.device_plan
                        assert dh.dtype == dn.dtype == torch.int32
                        assert dh.cpu().tolist() == hist
                        assert dn.cpu().tolist() == [s[2] for s in slots]
                    else:               # today's entries, today's bits
                        p = plain.batch(step, Bn, T=Tcut, lc=lc)
                        assert not hasattr(corpus, 'device_plan')
                        for x, y in ((b.audio, p.audio), (b.frames, p.frames),
                                     (b.rows, p.rows)):
                            assert (x is None and y is None) or \
                                torch.equal(x, y)
                        assert not b.history.any()
                for (u, st, n, _), h, o in zip(slots, hist, orig):
                    seen.add(('first', o == 0) if H else ('plain',))
                    if H:
                        seen.add(('clipped to the start', 0 < o < H))
                        seen.add(('cut below h', Tcut is not None and h == n
                                  and h > 0))
    assert {('first', True), ('first', False), ('clipped to the start', True),
            ('clipped to the start', False), ('cut below h', True),
            ('cut below h', False), ('plain',)} <= seen


def test_history_batch_through_a_model(hip_lib):
    """loss and every gradient with a history batch's frames window and
    offsets are, bit for bit, those with the whole utterances' frames at
    offset = start'; and the loss matches the float64 restatement's rule
    through the score: count = n - max(h, 1)."""
    from wavenet import WaveNetModel
    from wavenet.corpus import DeviceCorpus
    scales, Lc, Bn, size, H = (2, 2), GLC, 3, 37, 21
    utts, frames = _corpus_inputs()
    corpus = DeviceCorpus.from_arrays(utts, IDS, frames=frames, hop=GHOP,
                                      sample_size=size, seed=SEED, history=H)
    net = WaveNetModel(Bn, [1, 2, 4], 2, 32, 32, 64, quantization_channels=64,
                       use_biases=True, seed=3, local_condition_channels=Lc,
                       local_condition_upsample_scales=scales,
                       local_condition_context=2,
                       global_condition_channels=4,
                       global_condition_cardinality=4)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        net.params.copy_(0.3 * torch.randn(net.params.shape, generator=g))
    counts = [f.shape[0] for f in frames]
    with_history = 0
    for step in range(5):
        slots, hist, Tn, _ = hist_ref.plan(ULEN, size, 'pieces', SEED, step,
                                           Bn, H, IDS)
        if sum(s[2] - h for s, h in zip(slots, hist)) == 0 or Tn < 2:
            continue
        b = corpus.batch(step, Bn)
        gc = torch.from_numpy(b.gc)
        loss = float(net.loss(b.audio, gc, local_condition_batch=b.frames,
                              local_condition_offset=b.offsets,
                              lengths=b.lengths, history=b.history))
        torch.cuda.synchronize()
        grads = net.grads.clone()
        assert np.isfinite(loss) and bool(torch.isfinite(grads).all())
        need = max((s[1] + Tn - 1) // GHOP + 1 for s in slots)
        whole = np.zeros((Bn, max(need, max(counts)), Lc), np.float32)
        for j, s in enumerate(slots):
            whole[j, :counts[s[0]]] = frames[s[0]]
        ref = float(net.loss(R.gather(utts, slots, Tn), gc,
                             local_condition_batch=whole,
                             local_condition_offset=[s[1] for s in slots],
                             lengths=[s[2] for s in slots], history=hist))
        torch.cuda.synchronize()
        assert loss == ref, (step, loss, ref)
        assert torch.equal(grads, net.grads), step
        assert bool((grads != 0).any())
        s = net.score(b.audio, gc, local_condition_batch=b.frames,
                      local_condition_offset=b.offsets, lengths=b.lengths,
                      history=b.history)
        assert s.count.cpu().tolist() == \
            [n - max(h, 1) for (_, _, n, _), h in zip(slots, hist)]
        with_history += sum(h > 0 for h in hist)
    assert with_history


# ---- 12. command lines -----------------------------------------------------------
SMALL = {"filter_width": 2, "sample_rate": 16000,
         "dilations": [1, 2, 4, 8, 1, 2, 4, 8],
         "residual_channels": 32, "dilation_channels": 32,
         "quantization_channels": 256, "skip_channels": 64,
         "use_biases": True, "scalar_input": False,
         "initial_filter_width": 32, "residual_postproc": False}
# (longer than the trimming's 2048-sample frame)
SIZES = [3000, 2170, 2400, 2090]


def _wavs(d):
    os.makedirs(d)
    for i, n in enumerate(SIZES):
        t = np.arange(n) / 16000.0
        a = 0.5 * np.sin(2 * np.pi * (220 + 60 * i) * t + 0.3)
        wavfile.write(os.path.join(d, 'clip%d.wav' % i), 16000,
                      (a * 32767).astype(np.int16))


def test_train_and_evaluate_with_piece_history(hip_lib, tmp_path, capsys):
    import evaluate
    import train
    from wavenet import audio_reader as ar
    from wavenet.corpus import CorpusIndex
    params = str(tmp_path / 'params.json')
    json.dump(SMALL, open(params, 'w'))
    data = str(tmp_path / 'corpus')
    _wavs(data)
    logdir = str(tmp_path / 'run')
    common = ['--data_dir', data, '--batch_size', '2', '--wavenet_params',
              params, '--silence_threshold', '0']
    assert train.main(common + [
        '--logdir', logdir, '--num_steps', '3', '--checkpoint_every', '2',
        '--learning_rate', '0.002', '--device_corpus', 'true',
        '--sample_size', '64', '--piece_history', 'rf', '--validation_dir',
        data, '--validation_batches', '4']) == 0
    out = capsys.readouterr().out
    ev = [json.loads(l) for l in open(os.path.join(logdir, 'events.jsonl'))]
    steps = [e for e in ev if 'real_samples' in e]
    assert [e['step'] for e in steps] == [0, 1, 2]
    # the corpus's own pieces: sum(n - h) of every step's batch
    lengths = []
    for f in ar.find_files(data):
        a = ar.load_wav(f, 16000)
        lo, hi = ar.trim_bounds(a, 0.0)
        lengths.append(int(hi - lo))
    ix = CorpusIndex(lengths, None, 64, 'pieces', seed=train.CORPUS_SEED,
                     history=32)
    some = 0
    for e in steps:
        p = ix.plan(e['step'], 2)
        assert e['real_samples'] == int((p.n - p.history).sum()), e
        assert np.isfinite(e['loss'])
        assert re.search(r'^step %d - loss = \d+\.\d{3}, \(\d+\.\d{3} '
                         r'sec/step\), %d real samples$'
                         % (e['step'], e['real_samples']), out, re.M), e
        some += int(p.history.sum())
    assert some > 0
    ckpt = train.latest_checkpoint(logdir)
    stored = torch.load(ckpt, map_location='cpu')['device_corpus']
    assert stored['history'] == 32 and stored['sample_size'] == 64
    # held-out scoring with the same history: every sample but each file's
    # first is predicted exactly once
    assert evaluate.main([ckpt] + common[:2] + common[4:] + [
        '--sample_size', '64', '--piece_history', 'rf', '--batch_size',
        '16']) == 0
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert np.isfinite(res['bits_per_sample']) and res['bits_per_sample'] > 0
    assert res['samples'] == sum(lengths) - len(lengths)
    assert evaluate.main([ckpt] + common[:2] + common[4:] + [
        '--sample_size', '64', '--batch_size', '16']) == 0
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert plain['samples'] == sum(n - -(-n // 64) for n in lengths)
    assert plain['bits_per_sample'] != res['bits_per_sample']
    # the flag without --device_corpus true: argparse names it
    with pytest.raises(SystemExit):
        train.main(common + ['--logdir', logdir, '--piece_history', 'rf'])
    assert '--device_corpus true' in capsys.readouterr().err
