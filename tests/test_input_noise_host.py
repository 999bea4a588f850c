"""Input noise without a device (wavenet/input_noise.py): the argument
checks, the numpy reference against the Python-integer restatement of
tests/noise_ref.py, the rule's edge cases, the keys, the checkpoint form, the
new keywords, the two scripts' flags and the C entries' error codes."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import noise_ref as R
from wavenet import checkpoint, input_noise
from wavenet.input_noise import InputNoise, step_keys


@pytest.fixture
def untouched(monkeypatch):
    from wavenet import _lib

    def no(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'load', no)
    monkeypatch.setattr(_lib, 'require_gpu', no)


@pytest.mark.parametrize('args', [
    (-0.1, 2), (1.5, 2), (float('nan'), 2), (float('inf'), 2), (True, 2),
    (None, 2), ('0.5', 2), ([0.5], 2),
    (0.5, 0), (0.5, 4096), (0.5, -1), (0.5, 2.0), (0.5, True), (0.5, None),
    (0.5, 2, -1), (0.5, 2, 1 << 64), (0.5, 2, 1.0), (0.5, 2, None),
    (0.5, 2, True)])
def test_settings_are_checked_before_anything_is_touched(args, untouched):
    with pytest.raises(ValueError):
        InputNoise(*args)


def test_settings_thresholds_and_entry_round_trip():
    for prob, th in ((0, 0), (0.0, 0), (1, 1 << 24), (1.0, 1 << 24),
                     (0.5, 1 << 23), (2.0 ** -24, 1), (2.0 ** -25, 0),
                     (np.float32(0.25), 1 << 22), (0.1, 1677721)):
        assert InputNoise(prob, 1).thresh == th == R.thresh(prob)
    for args in ((0.5, 2), (1.0, 4095, (1 << 64) - 1), (0.0, 1, 7)):
        f = InputNoise(*args)
        e = f.entry()
        assert e == {'prob': float(args[0]), 'width': args[1],
                     'seed': args[2] if len(args) > 2 else 0}
        assert InputNoise.from_entry(e) == f
        assert InputNoise.from_entry(dict(e)) is not f
    assert InputNoise(0.5, 2) != InputNoise(0.5, 3)
    assert InputNoise(0.5, 2) != InputNoise(0.5, 2, 1)
    assert InputNoise.from_entry(None) is None
    for bad in ({}, {'prob': 0.5}, {'width': 2}, 0.5,
                {'prob': 2.0, 'width': 2}, {'prob': 0.5, 'width': 0}):
        with pytest.raises(ValueError):
            InputNoise.from_entry(bad)


def test_device_calls_check_their_arguments_first(untouched):
    f = InputNoise(0.5, 2)
    q = np.zeros((2, 5), np.int32)
    a = np.zeros((2, 5), np.float32)
    ok = [0, 1]
    for keys in ([0], [0, 1, 2], [0, -1], [0, 1 << 40], [0.0, 1.0],
                 [True, False], [[0, 1]], None):
        with pytest.raises(ValueError):
            f.codes(q, keys)
        with pytest.raises(ValueError):
            f.encode(a, 256, keys)
        with pytest.raises(ValueError):
            f.reference(q, keys, None, 256)
    for lengths in ([5], [0, 5], [5, 6], [1.0, 2.0]):
        with pytest.raises(ValueError):
            f.codes(q, ok, lengths)
        with pytest.raises(ValueError):
            f.encode(a, 256, ok, lengths)
        with pytest.raises(ValueError):
            f.reference(q, ok, lengths, 256)
    for bad in (np.zeros(5, np.int32), np.zeros((2, 0), np.int32),
                np.zeros((2, 5), np.float32), np.zeros((1, 2, 5), np.int32)):
        with pytest.raises(ValueError):
            f.codes(bad, ok)
    for bad in (np.zeros(5, np.float32), np.zeros((2, 5), np.int32),
                torch.zeros(2, 5, dtype=torch.int32)):
        with pytest.raises(ValueError):
            f.encode(bad, 256, ok)
    for Q in (1, 0, 2.0, None, True):
        with pytest.raises(ValueError):
            f.encode(a, Q, ok)
        with pytest.raises(ValueError):
            f.codes(q, ok, Q=Q)
    with pytest.raises(ValueError):
        f.codes(q, ok, out=torch.zeros(2, 5, dtype=torch.int32))   # host
    with pytest.raises(ValueError):
        f.encode(a, 256, ok, out=torch.zeros(2, 5, dtype=torch.int32))


def test_reference_equals_the_integer_restatement_over_the_grid():
    n = 0
    for _, q, keys, lengths, Q, prob, width, seed in R.grid():
        got = InputNoise(prob, width, seed).reference(q, keys, lengths, Q)
        want = R.codes_in(q, keys, lengths, Q, prob, width, seed)
        assert got.dtype == np.int32 and got.shape == q.shape
        assert np.array_equal(got, want), \
            (q.shape, keys, lengths, Q, prob, width, seed)
        n += 1
    assert n == 7 * 2 * 3 * 3 * 4 * 2


def test_splitmix64_restatement_has_the_published_value():
    assert R.splitmix64(0) == 0xe220a8397b1dcdaf
    hit, d = R.draw(0, 0, 0, 1.0, 4095)
    bits = R.splitmix64(R.TAG ^ R.splitmix64(0))
    assert hit and d == ((bits >> 24) & 0xFFFFF) % 4096 - (bits >> 44) % 4096


def test_prob_zero_is_the_identity_and_tiny_prob_hits_nothing_here():
    rng = np.random.default_rng(0)
    q = rng.integers(0, 256, (3, 1000)).astype(np.int32)
    keys = [0, 5, (1 << 40) - 1]
    for width in (1, 255, 4095):
        assert np.array_equal(InputNoise(0, width, 9).reference(
            q, keys, None, 256), q)
    big = np.full((3, 65536), 128, np.int32)
    assert np.array_equal(InputNoise(2.0 ** -24, 2, 1234).reference(
        big, keys, None, 256), big)
    assert np.array_equal(R.codes_in(big[:1, :4096], keys[:1], None, 256,
                                     2.0 ** -24, 2, 1234), big[:1, :4096])


def test_prob_one_full_width_hits_every_real_in_range_position():
    Q, B, T = 256, 3, 4000
    rng = np.random.default_rng(1)
    q = rng.integers(0, Q, (B, T)).astype(np.int32)
    q[0, 7], q[1, 9], q[2, 11] = -1, Q, 100000          # out of range
    n = np.array([T, 1234, 1])
    keys = [0, 5, (1 << 40) - 1]
    f = InputNoise(1, Q - 1, 3)
    r = f.reference(q, keys, n, Q)
    assert np.array_equal(r, R.codes_in(q, keys, n, Q, 1.0, Q - 1, 3))
    for b in range(B):
        assert np.array_equal(r[b, n[b]:], q[b, n[b]:])           # padding
        for t in range(n[b]):
            hit, d = R.draw(3, keys[b], t, 1.0, Q - 1)
            assert hit
            if 0 <= q[b, t] < Q:
                assert r[b, t] == min(max(q[b, t] + d, 0), Q - 1)
    assert (r[0, 7], r[1, 9], r[2, 11]) == (-1, Q, 100000)
    real = r[0][(q[0] >= 0) & (q[0] < Q)]
    assert real.min() == 0 and real.max() == Q - 1                # both clamps
    # d spans [-w, w]: more than half of the positions really move
    assert (r[0] != q[0]).mean() > 0.9
    # without lengths the whole row is real
    full = f.reference(q, keys, None, Q)
    assert np.array_equal(full[0], r[0]) and (full[2, 1:] != q[2, 1:]).any()


def test_statistics_of_the_reference():
    """Seed 1234, prob 0.5, width 2, 65536 positions, key 5, codes far from
    the clamps.  With prob 1 every position is hit: q_in - q is d itself,
    each value within 0.01 of (1, 2, 3, 2, 1) / 9.  With prob 0.5 a position
    moves iff it is hit and d != 0, and d is that of the prob-1 run: the hit
    rate, measured over the positions with d != 0, lies within 0.5 +- 0.01.
    (Measured: rates 0.4994 - 0.5013, d within 0.003: a threefold margin.)
    The mean and the variance of d: 65536 draws of variance 4 / 3 put the
    mean's standard error at 0.0045 and, with E d^4 = 4, the variance's at
    0.0058; the bars are four and five of those."""
    T = 65536
    q = np.full((1, T), 128, np.int32)
    d = InputNoise(1, 2, 1234).reference(q, [5], None, 256)[0] - 128
    for k, share in zip(range(-2, 3), (1, 2, 3, 2, 1)):
        got = float((d == k).mean())
        print('d = %+d: %.4f (want %.4f)' % (k, got, share / 9.0))
        assert abs(got - share / 9.0) <= 0.01
    assert abs(float(d.mean())) <= 0.02
    assert abs(float(d.var()) - 2 * (2 + 2) / 6.0) <= 0.03
    half = InputNoise(0.5, 2, 1234).reference(q, [5], None, 256)[0] - 128
    moved = half != 0
    assert np.array_equal(half[moved], d[moved])
    rate = float(moved[d != 0].mean())
    print('hit rate %.4f' % rate)
    assert abs(rate - 0.5) <= 0.01
    # the hits themselves, from the restatement
    hits = np.array([R.draw(1234, 5, t, 0.5, 2)[0] for t in range(T)])
    assert abs(float(hits.mean()) - 0.5) <= 0.01
    assert np.array_equal(moved, hits & (d != 0))


def test_step_keys_are_distinct_and_refuse_overflow():
    assert step_keys(3, 4, 1, 2).tolist() == [25, 27, 29, 31]
    assert step_keys(0, 2).tolist() == [0, 1]
    assert step_keys(0, 2).dtype == np.int64
    seen = set()
    for world in (3,):
        for step in range(5):
            for rank in range(world):
                k = step_keys(step, 4, rank, world).tolist()
                assert not seen & set(k) and len(set(k)) == 4
                seen |= set(k)
    assert seen == set(range(5 * 4 * 3))
    # a run resumed at step k draws the keys of the uninterrupted run
    assert step_keys(7, 8, 2, 4).tolist() == \
        [(7 * 8 + b) * 4 + 2 for b in range(8)]
    last = (1 << 40) - 1
    assert step_keys(last, 1).tolist() == [last]
    assert step_keys((1 << 37) - 1, 8).tolist()[-1] == last
    for bad in ((1 << 40, 1), (1 << 37, 8), ((1 << 39), 1, 1, 2)):
        with pytest.raises(ValueError, match='2\\*\\*40'):
            step_keys(*bad)
    for bad in ((-1, 2), (0, 0), (0, 2, 2, 2), (0, 2, -1, 2), (0, 2, 0, 0),
                (0.0, 2), (True, 2)):
        with pytest.raises(ValueError):
            step_keys(*bad)


def test_new_keywords_are_keyword_only_and_default_none():
    from wavenet import WaveNetModel
    for name, kws in (('loss', ('input_noise', 'noise_keys')),
                      ('score', ('input_noise', 'noise_keys')),
                      ('loss_from_codes', ('input_codes',)),
                      ('score_from_codes', ('input_codes',))):
        ps = inspect.signature(getattr(WaveNetModel, name)).parameters
        for kw in kws:
            assert ps[kw].kind is inspect.Parameter.KEYWORD_ONLY, (name, kw)
            assert ps[kw].default is None, (name, kw)
    ps = inspect.signature(checkpoint.save).parameters
    assert ps['input_noise'].default is None


def test_model_refusals_come_before_the_device(hip_lib, monkeypatch):
    """device='cpu' models compute nothing: what is refused here is refused
    before the check that a device is there, and without the library (which
    building a model loads)."""
    from wavenet import WaveNetModel, _lib
    kw = dict(batch_size=2, dilations=[1, 2], filter_width=2,
              residual_channels=8, dilation_channels=8, skip_channels=16,
              quantization_channels=16, device='cpu')
    net = WaveNetModel(**kw)
    scalar = WaveNetModel(scalar_input=True, initial_filter_width=4, **kw)

    def no(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'load', no)
    monkeypatch.setattr(_lib, 'require_gpu', no)
    a = np.zeros((2, 9), np.float32)
    f = InputNoise(0.5, 2)
    for call in (net.loss, net.score):
        with pytest.raises(ValueError, match='go together'):
            call(a, input_noise=f)
        with pytest.raises(ValueError, match='go together'):
            call(a, noise_keys=[0, 1])
        with pytest.raises(ValueError, match='InputNoise'):
            call(a, input_noise=(0.5, 2), noise_keys=[0, 1])
    q = torch.zeros(2, 9, dtype=torch.int32)
    for call in (lambda: scalar.loss(a, input_noise=f, noise_keys=[0, 1]),
                 lambda: scalar.score(a, input_noise=f, noise_keys=[0, 1]),
                 lambda: scalar.loss_from_codes(q, input_codes=q),
                 lambda: scalar.score_from_codes(q, input_codes=q)):
        with pytest.raises(ValueError, match='float audio, not the codes'):
            call()


def test_the_scripts_parse_the_flags(capsys):
    import evaluate
    import train
    ev = ['ck', '--data_dir', 'd']
    for parse, argv in ((train.get_arguments, ['--synthetic']),
                        (evaluate.get_arguments, ev)):
        a = parse(argv)
        assert a.input_noise is None and a.input_noise_seed is None
        assert a.noise is None
        a = parse(argv + ['--input_noise', '0.5,2'])
        assert a.noise == InputNoise(0.5, 2, 0)
        a = parse(argv + ['--input_noise', '1,255', '--input_noise_seed',
                          str((1 << 64) - 1)])
        assert a.noise == InputNoise(1.0, 255, (1 << 64) - 1)
        assert parse(argv + ['--input_noise', '0,1']).noise.thresh == 0
        capsys.readouterr()
        for bad in ('0.5', '0.5,2,3', 'a,2', '0.5,b', '0.5,2.5', '1.5,2',
                    '-0.1,2', 'nan,2', '0.5,0', '0.5,4096', ''):
            with pytest.raises(SystemExit):
                parse(argv + ['--input_noise', bad])
            assert '--input_noise' in capsys.readouterr().err, bad
        for bad in ('-1', str(1 << 64)):
            with pytest.raises(SystemExit):
                parse(argv + ['--input_noise', '0.5,2', '--input_noise_seed',
                              bad])
            assert '--input_noise_seed' in capsys.readouterr().err
        with pytest.raises(SystemExit):
            parse(argv + ['--input_noise_seed', '3'])
        assert '--input_noise' in capsys.readouterr().err
    assert input_noise.parse_flag('0.25,7') == (0.25, 7)


def test_save_writes_the_entry_only_where_given(tmp_path):
    class Net(object):
        def state_dict(self):
            return {}
    entry = InputNoise(0.5, 2, 11).entry()
    checkpoint.save(Net(), str(tmp_path / 'a'), 3, input_noise=entry)
    checkpoint.save(Net(), str(tmp_path / 'b'), 3)
    a = torch.load(str(tmp_path / 'a' / 'model.ckpt-3'))
    b = torch.load(str(tmp_path / 'b' / 'model.ckpt-3'))
    assert a['input_noise'] == {'prob': 0.5, 'width': 2, 'seed': 11}
    assert InputNoise.from_entry(a['input_noise']) == InputNoise(0.5, 2, 11)
    assert 'input_noise' not in b
    assert sorted(b) == ['step', 'variables']


def test_workspace_views_share_q_tgt_with_their_owner(hip_lib):
    from wavenet import WaveNetModel, workspace
    net = WaveNetModel(batch_size=2, dilations=[1, 2], filter_width=2,
                       residual_channels=32, dilation_channels=32,
                       skip_channels=64, quantization_channels=64,
                       device='cpu')
    owner = workspace.get(net, 2, 500, True)
    for training in (True, False):
        view = workspace.get(net, 2, 123, training)
        assert view.capacity == owner.N
        assert view.q_tgt.data_ptr() == owner.q_tgt.data_ptr()
        assert view.q_tgt.dtype == torch.int32 and view.q_tgt.numel() == 246
    assert owner.q_tgt.numel() == owner.q.numel() == 1000
    assert owner.q_tgt.data_ptr() != owner.q.data_ptr()


def test_entry_points_validate_without_a_device(hip_lib):
    """wn_code_noise / wn_mu_law_encode_noisy: every check comes before a
    launch."""
    from wavenet import _lib
    assert _lib.SIGNATURES['wn_code_noise'][1][7] is _lib.c_u64
    assert _lib.SIGNATURES['wn_mu_law_encode_noisy'][1][9] is _lib.c_u64
    buf = (ctypes.c_int64 * 64)()
    a = ctypes.addressof(buf)
    b, k = a + 128, a + 256
    noise, fused = hip_lib.wn_code_noise, hip_lib.wn_mu_law_encode_noisy
    T24 = 1 << 24

    def n(codes=a, codes_in=b, keys=k, lengths=None, B=1, T=8, Q=256,
          thresh=5, width=2):
        return noise(codes, codes_in, keys, lengths, B, T, Q, 7, thresh,
                     width, None)

    def f(audio=a, codes=b, codes_in=b + 64, keys=k, lengths=None, B=1, T=8,
          thr=k + 64, Q=256, thresh=5, width=2):
        return fused(audio, codes, codes_in, keys, lengths, B, T, thr, Q, 7,
                     thresh, width, None)
    for call in (n, f):
        for name in ('codes', 'codes_in', 'keys'):
            assert call(**{name: None}) == -5, name
        for bad in (dict(B=0), dict(T=0), dict(B=-1), dict(T=T24 + 1),
                    dict(Q=1), dict(width=0), dict(width=4096),
                    dict(thresh=-1), dict(thresh=T24 + 1)):
            assert call(**bad) == -1, bad
        assert call(codes=a + 2) == -3 and call(codes_in=b + 1) == -3
        assert call(keys=k + 4) == -3 and call(lengths=a + 2) == -3
    assert f(audio=None) == -5 and f(thr=None) == -5
    assert f(audio=a + 1) == -3 and f(thr=k + 66) == -3
    assert f(codes=b, codes_in=b) == -2
