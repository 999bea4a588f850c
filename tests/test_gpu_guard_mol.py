"""Guard bands (tests/guard.py) around every operand of the entries of
include/wavenet_mol.h that write through a pointer: nothing outside the
operands is read or written -- poisoned margins round the logits (padded rows:
the gap columns belong to the band), the levels, the lengths, starts and
1 / den, the outputs; the padded columns k >= K INSIDE the logits and the
audio behind n[b] are poison too, so no output depends on them.
tests/test_mol_host.py holds ENTRIES against the header."""
import numpy as np
import pytest
import torch

import guard
import mol_cases as MC
import mol_ref as R

pytestmark = pytest.mark.gpu

# the entries of wavenet_mol.h that write through a pointer
ENTRIES = ('wn_mol_quantize', 'wn_mol_loss', 'wn_mol_score',
           'wn_mol_params_row', 'wn_mol_sample')


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _body_free(bits):
    return not (bits == guard._signed(guard.BODY32, 32)).any()


@pytest.mark.parametrize('B,T,skew', [(3, 37, 0), (1, 65, 4), (2, 300, 8)])
def test_quantize_stays_inside_its_operands(hip_lib, B, T, skew):
    from wavenet import mol
    rng = np.random.default_rng(T)
    y = rng.uniform(-1.1, 1.1, (B, T)).astype(np.float32)
    n = rng.integers(0, T + 1, B).astype(np.int32)
    for b in range(B):
        y[b, n[b]:] = np.nan
    ar = guard.Arena('cuda')
    ar.place('audio', y, torch.float32, skew_bytes=skew)
    ar.place('lengths', n, torch.int32, fill=(T, 0), skew_bytes=skew)
    ar.place('levels', (B, T), torch.int32, role='out', skew_bytes=skew)
    ar.place('centres', (B, T), torch.float32, role='out', skew_bytes=skew)

    def run():
        assert hip_lib.wn_mol_quantize(
            ar.ptr('audio'), ar.ptr('lengths'), ar.ptr('levels'),
            ar.ptr('centres'), B, T, _stream()) == 0
    bits = guard.read_check(ar, run)
    wl, wc = mol.levels_reference(y, n)
    assert torch.equal(bits['levels'].cpu(), torch.from_numpy(wl))
    assert torch.equal(bits['centres'].cpu(), torch.from_numpy(wc.view(np.int32)))


# (B, T, K, ld - 3 Kp, skew bytes, in place, with starts / lengths / 1 / den)
LOSS_CASES = [(3, 37, 10, 4, 0, False, True), (1, 65, 1, 0, 0, True, False),
              (2, 64, 32, 8, 0, True, True), (1, 63, 4, 0, 0, False, False),
              (5, 200, 5, 4, 0, False, True)]


@pytest.mark.parametrize('B,T,K,gap,skew,in_place,masked', LOSS_CASES)
def test_loss_stays_inside_its_operands(hip_lib, B, T, K, gap, skew, in_place,
                                        masked):
    lg, lv = MC.kernel_case(B, T, K, gap)
    Kp, ld = MC.padded(K), 3 * MC.padded(K) + gap
    nparts = hip_lib.wn_xent_partials(B * T)
    rng = np.random.default_rng(K)
    ar = guard.Arena('cuda')
    ar.place('logits', lg[:, :3 * Kp], torch.float32,
             ld=ld if gap else None, role='inout' if in_place else 'in')
    ar.place('levels', lv, torch.int32, fill=(65535, 0), skew_bytes=4)
    if masked:
        ar.place('starts', rng.integers(0, 5, B).astype(np.int32),
                 torch.int32, fill=(0, T))
        ar.place('lengths', rng.integers(1, T + 1, B).astype(np.int32),
                 torch.int32, fill=(T, 1))
        ar.place('inv', np.array([1.0 / 77], np.float32), torch.float32)
    if not in_place:
        ar.place('dlogits', (B * T, 3 * Kp), torch.float32, role='out',
                 ld=ld if gap else None)
    ar.place('parts', (nparts,), torch.float32, role='out')
    dst = 'logits' if in_place else 'dlogits'
    m = (lambda k: ar.ptr(k)) if masked else (lambda k: None)

    def run():
        assert hip_lib.wn_mol_loss(
            ar.ptr('logits'), ld, ar.ptr('levels'), m('starts'), m('lengths'),
            m('inv'), ar.ptr(dst), ar.ptr('parts'), B, T, K, MC.LSM,
            _stream()) == 0
    bits = guard.read_check(ar, run)
    ar.check()
    assert _body_free(bits['parts']) and _body_free(bits[dst])
    got = bits[dst].cpu().numpy().view(np.float32)
    assert np.isfinite(got).all()


@pytest.mark.parametrize('B,T,K,gap,skew,in_place,masked', LOSS_CASES)
def test_score_stays_inside_its_operands(hip_lib, B, T, K, gap, skew, in_place,
                                         masked):
    lg, lv = MC.kernel_case(B, T, K, gap)
    Kp, ld = MC.padded(K), 3 * MC.padded(K) + gap
    rng = np.random.default_rng(K)
    ar = guard.Arena('cuda')
    ar.place('logits', lg[:, :3 * Kp], torch.float32, ld=ld if gap else None)
    ar.place('levels', lv, torch.int32, fill=(65535, 0), skew_bytes=4)
    if masked:
        ar.place('starts', rng.integers(0, 5, B).astype(np.int32),
                 torch.int32, fill=(0, T))
        ar.place('lengths', rng.integers(1, T + 1, B).astype(np.int32),
                 torch.int32, fill=(T, 1))
    rows = not in_place                  # (with and without row_nll)
    if rows:
        ar.place('row_nll', (B, T), torch.float32, role='out')
    ar.place('clip_nll', (B,), torch.float64, role='out')
    ar.place('clip_count', (B,), torch.int32, role='out')
    ar.place('scratch', (hip_lib.wn_mol_score_scratch_floats(B * T),),
             torch.float32, role='out')
    m = (lambda k: ar.ptr(k)) if masked else (lambda k: None)

    def run():
        assert hip_lib.wn_mol_score(
            ar.ptr('logits'), ld, ar.ptr('levels'), m('starts'), m('lengths'),
            ar.ptr('row_nll') if rows else None, ar.ptr('clip_nll'),
            ar.ptr('clip_count'), ar.ptr('scratch'), B, T, K, MC.LSM,
            _stream()) == 0
    bits = guard.read_check(ar, run)
    ar.check()
    assert not (bits['clip_nll'] == guard._signed(guard.BODY64, 64)).any()
    if rows:
        assert _body_free(bits['row_nll'])


@pytest.mark.parametrize('K,skew', [(1, 0), (10, 4), (32, 8)])
def test_params_row_stays_inside_its_operands(hip_lib, K, skew):
    from wavenet import mol
    lg, _ = MC.kernel_case(1, 4, K)
    ar = guard.Arena('cuda')
    ar.place('row', lg[2], torch.float32, skew_bytes=skew)
    ar.place('out', (3, K), torch.float32, role='out', skew_bytes=skew)

    def run():
        assert hip_lib.wn_mol_params_row(ar.ptr('row'), K, MC.LSM,
                                         ar.ptr('out'), _stream()) == 0
    bits = guard.read_check(ar, run)
    want = mol.params_reference(lg[2], K, MC.LSM)
    assert torch.equal(bits['out'].cpu(), torch.from_numpy(want.view(np.int32)))


@pytest.mark.parametrize('K,R_,skew', [(1, 1, 0), (10, 65, 4), (32, 96, 8)])
def test_sample_stays_inside_its_operands(hip_lib, K, R_, skew):
    from wavenet import mol
    p, seeds, counters = MC.sample_fixture(K)
    p, seeds, counters = p[:R_], seeds[:R_], counters[:R_]
    ar = guard.Arena('cuda')
    ar.place('params', p, torch.float32, skew_bytes=skew)
    ar.place('seeds', seeds, torch.int64, skew_bytes=skew & 8)
    ar.place('counters', counters, torch.int64, skew_bytes=skew & 8)
    ar.place('levels', (R_,), torch.int32, role='out', skew_bytes=skew)
    ar.place('centres', (R_,), torch.float32, role='out', skew_bytes=skew)

    def run():
        assert hip_lib.wn_mol_sample(
            ar.ptr('params'), ar.ptr('seeds'), ar.ptr('counters'), 0.7,
            ar.ptr('levels'), ar.ptr('centres'), R_, K, _stream()) == 0
    bits = guard.read_check(ar, run)
    wl, wc = mol.sample_reference(p, seeds, counters, 0.7)
    assert torch.equal(bits['levels'].cpu(), torch.from_numpy(wl))
    assert torch.equal(bits['centres'].cpu(), torch.from_numpy(wc.view(np.int32)))
