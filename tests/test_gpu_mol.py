"""csrc/wn_mol.hip alone, on synthetic head outputs (tests/mol_cases.py): the
row loss and every gradient against float64 (tests/mol_ref.py), held to four
times the larger of a numpy float32 restatement's own error and one float32
ulp of the output's scale (mol_cases.worst_ratio: both measured when the test
runs); the bit-for-bit properties; exact zeros; the level, parameter and
sampling rules bit for bit."""
import numpy as np
import pytest
import torch

import mol_cases as MC
import mol_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 63), (1, 64), (1, 65), (3, 37)]
KS = [1, 4, 10, 32]


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def run_loss(lib, lg, lv, K, lsm=MC.LSM, starts=None, lengths=None, inv=None,
             mode='out'):
    """(loss sum, dlogits numpy or None) of wn_mol_loss.  mode: 'out' (a
    second buffer), 'in' (in place) or 'fwd' (no gradient)."""
    B, T = lv.shape
    ld = lg.shape[1]
    d_lg, d_lv = _dev(lg), _dev(lv, torch.int32)
    d_s = None if starts is None else _dev(starts, torch.int32)
    d_n = None if lengths is None else _dev(lengths, torch.int32)
    d_inv = None if inv is None else _dev(np.array([inv], np.float32))
    parts = torch.full((lib.wn_xent_partials(B * T),), float('nan'),
                       device='cuda')
    out = None
    if mode == 'out':
        out = torch.full_like(d_lg, 123.0)
    elif mode == 'in':
        out = d_lg
    p = lambda t: None if t is None else t.data_ptr()
    code = lib.wn_mol_loss(p(d_lg), ld, p(d_lv), p(d_s), p(d_n), p(d_inv),
                           p(out), p(parts), B, T, K, lsm, _st())
    assert code == 0, code
    torch.cuda.synchronize()
    return parts.cpu().numpy(), None if out is None else out.cpu().numpy()


def run_score(lib, lg, lv, K, lsm=MC.LSM, starts=None, lengths=None):
    B, T = lv.shape
    d_lg, d_lv = _dev(lg), _dev(lv, torch.int32)
    d_s = None if starts is None else _dev(starts, torch.int32)
    d_n = None if lengths is None else _dev(lengths, torch.int32)
    rows = torch.full((B, T), float('nan'), device='cuda')
    nll = torch.empty(B, dtype=torch.float64, device='cuda')
    cnt = torch.empty(B, dtype=torch.int32, device='cuda')
    scr = torch.empty(lib.wn_mol_score_scratch_floats(B * T), device='cuda')
    p = lambda t: None if t is None else t.data_ptr()
    code = lib.wn_mol_score(p(d_lg), lg.shape[1], p(d_lv), p(d_s), p(d_n),
                            p(rows), p(nll), p(cnt), p(scr), B, T, K, lsm,
                            _st())
    assert code == 0, code
    torch.cuda.synchronize()
    return rows.cpu().numpy(), nll.cpu().numpy(), cnt.cpu().numpy()


_worst = {}


@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('gap', [0, 4])
@pytest.mark.parametrize('B,T', SHAPES)
def test_loss_and_gradients_against_float64(hip_lib, B, T, K, gap):
    from wavenet import mol
    lg, lv = MC.kernel_case(B, T, K, gap)
    Kp, N = MC.padded(K), B * T
    tgt = R.targets(lv).reshape(-1)
    inv = float(np.float32(1.0) / np.float32(N))
    n64, g64 = R.loss_rows(lg[:, :3 * Kp], tgt, K, MC.LSM, inv)
    n32, g32 = mol.loss_reference(lg, tgt, K, MC.LSM, inv, dtype=np.float32)
    parts, dl = run_loss(hip_lib, lg, lv, K)
    rows, clip, cnt = run_score(hip_lib, lg, lv, K)
    assert np.isfinite(parts).all() and np.isfinite(rows).all()
    assert np.isfinite(dl[:, :3 * Kp]).all()
    # the gap columns are not written
    assert (dl[:, 3 * Kp:] == 123.0).all()
    sc = MC.scales(lg, tgt, K, MC.LSM, inv)
    has = tgt >= 0
    ratios = {'nll': 0.0}
    if has.any():
        ratios['nll'] = MC.worst_ratio(rows.reshape(-1)[has], n32[has],
                                       n64[has], sc['nll'][has])
        for blk, name in enumerate(('pi', 'mu', 'beta')):
            cols = slice(blk * Kp, blk * Kp + K)
            ratios[name] = MC.worst_ratio(dl[has][:, cols], g32[has][:, cols],
                                          np.nan_to_num(g64[has][:, cols]),
                                          sc[name][has])
    # the loss: the sum of the rows, each within its bound
    total = float(parts.astype(np.float64).sum())
    want = float(n64.sum())
    bound = 4.0 * (np.abs(n32.astype(np.float64) - n64).sum() +
                   N * MC.ulp32(max(1.0, np.abs(n64).sum())))
    ratios['loss'] = abs(total - want) / bound
    for k, v in ratios.items():
        _worst[k] = max(_worst.get(k, 0.0), v)
    print('mol kernel B=%d T=%d K=%d gap=%d: worst error / bound %s; so far %s'
          % (B, T, K, gap, {k: round(v, 3) for k, v in ratios.items()},
             {k: round(v, 3) for k, v in _worst.items()}))
    assert max(ratios.values()) <= 1.0, ratios
    # exact zeros: padded columns, rows without a target
    for blk in range(3):
        assert (dl[:, blk * Kp + K:(blk + 1) * Kp] == 0).all()
    assert (dl[~has][:, :3 * Kp] == 0).all() and (rows.reshape(-1)[~has] == 0).all()
    assert np.array_equal(cnt, has.reshape(B, T).sum(1))
    assert np.abs(clip - rows.astype(np.float64).sum(1)).max() <= \
        1e-12 * max(1.0, np.abs(clip).max())


@pytest.mark.parametrize('K', [1, 10, 32])
def test_bit_for_bit_properties(hip_lib, K):
    B, T = 3, 37
    lg, lv = MC.kernel_case(B, T, K, 4)
    inv = 1.0 / 55.0
    full = np.full(B, T, np.int32)
    p0, out = run_loss(hip_lib, lg, lv, K, lengths=full, inv=inv)
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.int32)
    W = 3 * MC.padded(K)
    # in place equals out of place; forward only gives the same partials
    p1, inp = run_loss(hip_lib, lg, lv, K, lengths=full, inv=inv, mode='in')
    p2, _ = run_loss(hip_lib, lg, lv, K, lengths=full, inv=inv, mode='fwd')
    assert np.array_equal(bits(out[:, :W]), bits(inp[:, :W]))
    assert np.array_equal(bits(p0), bits(p1)) and np.array_equal(bits(p0), bits(p2))
    # lengths = None equals full lengths (at the same 1 / den), and starts = 0
    # equals no starts
    _, a = run_loss(hip_lib, lg, lv, K, inv=inv)
    _, b = run_loss(hip_lib, lg, lv, K, lengths=full, inv=inv,
                    starts=np.zeros(B, np.int32))
    assert np.array_equal(bits(a[:, :W]), bits(out[:, :W]))
    assert np.array_equal(bits(b[:, :W]), bits(out[:, :W]))
    rows_all, _, _ = run_score(hip_lib, lg, lv, K)
    # a clip alone equals the clip in the batch at the same 1 / den: gradient
    # rows and scored rows
    for c in range(B):
        _, one = run_loss(hip_lib, lg[c * T:(c + 1) * T], lv[c:c + 1], K,
                          inv=inv)
        assert np.array_equal(bits(one[:, :W]), bits(out[c * T:(c + 1) * T, :W]))
        r1, _, _ = run_score(hip_lib, lg[c * T:(c + 1) * T], lv[c:c + 1], K)
        assert np.array_equal(bits(r1[0]), bits(rows_all[c]))
    # ragged lengths and a history: the rows with a target keep their bits,
    # the others are exact zeros; the loss rows are the scored rows
    n = np.array([37, 20, 1], np.int32)
    h = np.array([0, 7, 0], np.int32)
    parts, d = run_loss(hip_lib, lg, lv, K, starts=h, lengths=n, inv=inv)
    rows, clip, cnt = run_score(hip_lib, lg, lv, K, starts=h, lengths=n)
    tgt = R.targets(lv, n, h)
    has = (tgt >= 0).reshape(-1)
    assert np.array_equal(bits(d[has][:, :W]), bits(out[has][:, :W]))
    assert (d[~has][:, :W] == 0).all()
    assert np.array_equal(bits(rows.reshape(-1)[has]),
                          bits(rows_all.reshape(-1)[has]))
    assert (rows.reshape(-1)[~has] == 0).all()
    assert cnt.tolist() == [36, 13, 0]
    assert abs(float(parts.astype(np.float64).sum()) - clip.sum()) <= \
        1e-5 * max(1.0, abs(clip.sum()))


def test_many_tiles_and_every_partial(hip_lib):
    """More tiles than one pass of the grid covers leave rows out nowhere: 5000
    rows are 79 tiles over 1024 workgroups; 70000 rows 1094 tiles."""
    from wavenet import mol
    for B, T in ((1, 5000), (7, 10000)):
        K = 4
        lg, lv = MC.kernel_case(B, T, K)
        tgt = R.targets(lv).reshape(-1)
        parts, dl = run_loss(hip_lib, lg, lv, K)
        # (against the package's float64 statement of the rule: the kernel's
        # outputs are its values rounded to float32 once, 6e-8 of an entry)
        n64, g64 = mol.loss_reference(lg, tgt, K, MC.LSM,
                                      np.float32(1.0) / np.float32(B * T))
        assert np.isfinite(parts).all() and np.isfinite(dl).all()
        assert abs(parts.astype(np.float64).sum() - n64.sum()) \
            <= 1e-6 * n64.sum()
        scale = np.abs(g64).max(1, keepdims=True)
        assert (np.abs(dl - g64) <= 1e-6 * scale).all()
        assert len(parts) == hip_lib.wn_xent_partials(B * T)


@pytest.mark.parametrize('B,T', [(1, 1), (3, 37), (2, 1000)])
def test_quantize_bit_for_bit(hip_lib, B, T):
    from wavenet import mol
    rng = np.random.default_rng(T)
    y = rng.uniform(-1.2, 1.2, (B, T)).astype(np.float32)
    y.reshape(-1)[::11] = rng.choice(
        np.array([-1, 1, 0, -0.0, np.nan, 1e30, -1e30], np.float32), y.reshape(-1)[::11].size)
    j = rng.integers(0, 65535, y.reshape(-1)[1::13].size)
    y.reshape(-1)[1::13] = ((2 * j + 1) / 65535.0 - 1.0).astype(np.float32)
    for lengths in (None, rng.integers(0, T + 1, B).astype(np.int32)):
        d_y = _dev(y)
        lv = torch.full((B, T), -7, dtype=torch.int32, device='cuda')
        ce = torch.full((B, T), float('nan'), device='cuda')
        d_n = None if lengths is None else _dev(lengths)
        poisoned = y.copy()
        if lengths is not None:          # behind n[b] nothing is read
            for b in range(B):
                poisoned[b, lengths[b]:] = np.nan
            d_y = _dev(poisoned)
        assert hip_lib.wn_mol_quantize(
            d_y.data_ptr(), None if d_n is None else d_n.data_ptr(),
            lv.data_ptr(), ce.data_ptr(), B, T, _st()) == 0
        wl, wc = mol.levels_reference(poisoned, lengths)
        assert np.array_equal(lv.cpu().numpy(), wl)
        assert np.array_equal(ce.cpu().numpy().view(np.int32), wc.view(np.int32))
        # centres over the audio itself
        assert hip_lib.wn_mol_quantize(
            d_y.data_ptr(), None if d_n is None else d_n.data_ptr(),
            lv.data_ptr(), d_y.data_ptr(), B, T, _st()) == 0
        assert np.array_equal(d_y.cpu().numpy().view(np.int32), wc.view(np.int32))


@pytest.mark.parametrize('K', KS)
def test_params_row_bit_for_bit(hip_lib, K):
    from wavenet import mol
    lg, _ = MC.kernel_case(1, 9, K)
    for row in lg:
        out = torch.full((3, K), float('nan'), device='cuda')
        assert hip_lib.wn_mol_params_row(_dev(row).data_ptr(), K, MC.LSM,
                                         out.data_ptr(), _st()) == 0
        want = mol.params_reference(row, K, MC.LSM)
        assert np.array_equal(out.cpu().numpy().view(np.int32),
                              want.view(np.int32))
        assert np.abs(want - R.params(row, K, MC.LSM)).max() < 1e-6


@pytest.mark.parametrize('K', MC.SAMPLE_K)
@pytest.mark.parametrize('tau', MC.SAMPLE_TEMPERATURES)
def test_sample_equals_the_reference(hip_lib, K, tau):
    """Exact, with nothing left out: tests/test_mol_host.py shows that no
    fixture draw lies near a rounding boundary."""
    from wavenet import mol
    p, seeds, counters = MC.sample_fixture(K)
    lv, ce = mol.sample(_dev(p), seeds, counters, tau)
    wl, wc = mol.sample_reference(p, seeds, counters, tau)
    assert np.array_equal(lv.cpu().numpy(), wl)
    assert np.array_equal(ce.cpu().numpy().view(np.int32), wc.view(np.int32))
    # a row's draw does not depend on its neighbours
    one = mol.sample(_dev(p[5:6]), seeds[5:6], counters[5:6], tau)
    assert int(one[0][0]) == wl[5]
