"""Pre-emphasis / de-emphasis without a device (wavenet/emphasis.py): the
alpha checks, the numpy references and their round trip, the checkpoint form,
the three scripts' --preemphasis flag and the aliasing refusal."""
import os

import numpy as np
import pytest
import torch

import emph_ref as R
from wavenet import checkpoint
from wavenet.emphasis import DeStream, Emphasis, from_cli


@pytest.mark.parametrize('alpha', [-0.1, 1.0, 1.5, True, False, float('nan'),
                                   float('inf'), None, '0.97', [0.97],
                                   1.0 - 1e-9])
def test_alpha_is_checked_before_anything_is_touched(alpha, monkeypatch):
    from wavenet import _lib

    def no(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'load', no)
    monkeypatch.setattr(_lib, 'require_gpu', no)
    with pytest.raises(ValueError):
        Emphasis(alpha)


def test_alpha_values_and_entry_round_trip():
    for a in (0, 0.0, 0.5, 0.97, np.float32(0.97), 0.995):
        f = Emphasis(a)
        assert f.alpha == float(a) and f.alpha32 == np.float32(a)
        assert f.entry() == {'alpha': float(a)}
        assert Emphasis.from_entry(f.entry()) == f
    assert Emphasis(0.97).entry() == {'alpha': 0.97}
    assert Emphasis.from_entry(None) is None
    assert Emphasis(0.97) != Emphasis(0.5)
    for bad in ({}, {'beta': 1}, 0.97, {'alpha': 2.0}):
        with pytest.raises(ValueError):
            Emphasis.from_entry(bad)


def test_reference_pre_is_two_float32_roundings():
    rng = np.random.default_rng(0)
    x = rng.uniform(-1, 1, (3, 400)).astype(np.float32)
    f = Emphasis(0.97)
    e = f.reference_pre(x)
    a = np.float32(0.97)
    assert e.dtype == np.float32 and e.shape == x.shape
    assert np.array_equal(e[:, 0], x[:, 0])
    for b, t in ((0, 1), (1, 57), (2, 399)):
        assert e[b, t] == np.float32(x[b, t] - np.float32(a * x[b, t - 1]))
    n = np.array([400, 1, 123])
    en = f.reference_pre(x, n)
    for b in range(3):
        assert np.array_equal(en[b, :n[b]], e[b, :n[b]])
        assert not en[b, n[b]:].any()
    assert np.array_equal(f.reference_pre(x[1]), e[1])
    assert np.abs(e).max() > 1.0                   # (it may leave [-1, 1])
    z = Emphasis(0)
    assert z.reference_pre(x).tobytes() == x.tobytes()
    assert z.reference_de(x).tobytes() == x.tobytes()


@pytest.mark.parametrize('alpha', [0.5, 0.97, 0.995])
def test_references_round_trip_within_the_bound(alpha):
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, (2, 3000)).astype(np.float32)
    f = Emphasis(alpha)
    e = f.reference_pre(x)
    y = f.reference_de(e)
    assert y.dtype == np.float32
    # the sequential float32 loop against the float64 recurrence of e ...
    y64, bound = R.de64(e, alpha)
    assert (np.abs(y - y64) <= bound).all()
    # ... which is x up to pre's two roundings per sample, filtered
    slack = R.de64(2.0 ** -23 * (np.abs(x) + np.abs(e)), alpha)[0]
    assert (np.abs(y64 - x) <= slack).all()
    assert np.abs(y - x).max() < 1e-4
    # lengths, initial and pieces
    n = np.array([3000, 1234])
    yn = f.reference_de(e, n)
    assert np.array_equal(yn[1, :1234], y[1, :1234]) and not yn[1, 1234:].any()
    tail = f.reference_de(e[:, 1000:], initial=y[:, 999])
    assert tail.tobytes() == y[:, 1000:].tobytes()


def test_bound_recurrences_are_the_sums():
    rng = np.random.default_rng(2)
    e = rng.uniform(-1, 1, 40)
    a = R.alpha64(0.97)
    y, bound = R.de64(e, 0.97, initial=[0.3])
    for t in (0, 1, 17, 39):
        k = np.arange(t + 1)
        want_y = (a ** k * e[t - k]).sum() + a ** (t + 1) * 0.3
        want_b = ((2 * k + 3) * a ** k * np.abs(e[t - k])).sum() + \
            (2 * (t + 1) + 3) * a ** (t + 1) * 0.3
        assert abs(y[t] - want_y) < 1e-12
        assert abs(bound[t] - (2.0 ** -24 * want_b + 2.0 ** -126)) < 1e-18


def test_pre_refuses_out_is_audio_before_the_device(monkeypatch):
    from wavenet import _lib

    def no(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'load', no)
    monkeypatch.setattr(_lib, 'require_gpu', no)
    x = torch.zeros(2, 50)
    with pytest.raises(ValueError, match='out must not be audio'):
        Emphasis(0.97).pre(x, out=x)
    for bad in (np.zeros((2, 3), np.int32), np.zeros((2, 3, 4), np.float32),
                np.zeros((0,), np.float32)):
        with pytest.raises(ValueError):
            Emphasis(0.97).pre(bad)
        with pytest.raises(ValueError):
            Emphasis(0.97).de(bad)
    with pytest.raises(ValueError):
        Emphasis(0.97).pre(np.zeros((2, 9), np.float32), lengths=[3, 10])
    with pytest.raises(ValueError):
        Emphasis(0.97).de(np.zeros((2, 9), np.float32), initial=[1.0])


def test_from_cli_defaults_override_and_continued_mismatch():
    stored = {'alpha': 0.97}
    assert from_cli(None, None) is None
    assert from_cli(None, stored) == Emphasis(0.97)
    assert from_cli(0.9, stored) == Emphasis(0.9)          # the flag overrides
    assert from_cli(0.0, stored) is None                   # 0 switches it off
    assert from_cli(0.5, None) == Emphasis(0.5)
    # a run continued in its logdir keeps its value
    assert from_cli(None, stored, continued=True) == Emphasis(0.97)
    assert from_cli(0.97, stored, continued=True) == Emphasis(0.97)
    assert from_cli(0.0, None, continued=True) is None
    with pytest.raises(ValueError) as e:
        from_cli(0.9, stored, continued=True)
    assert '0.9' in str(e.value) and '0.97' in str(e.value)
    with pytest.raises(ValueError) as e:
        from_cli(0.0, stored, continued=True)
    assert '0.0' in str(e.value) and '0.97' in str(e.value)
    with pytest.raises(ValueError) as e:
        from_cli(0.5, None, continued=True)
    assert '0.5' in str(e.value) and '0.0' in str(e.value)
    with pytest.raises(ValueError):
        from_cli(1.5, stored)


def test_the_scripts_parse_the_flag(tmp_path, capsys):
    import evaluate
    import generate
    import train
    assert train.get_arguments(['--synthetic']).preemphasis is None
    assert train.get_arguments(['--synthetic', '--preemphasis', '0.97']
                               ).preemphasis == 0.97
    assert generate.get_arguments(['ck']).preemphasis is None
    assert generate.get_arguments(['ck', '--preemphasis', '0']
                                  ).preemphasis == 0.0
    ev = ['ck', '--data_dir', 'd']
    assert evaluate.get_arguments(ev).preemphasis is None
    assert evaluate.get_arguments(ev + ['--preemphasis', '0.5']
                                  ).preemphasis == 0.5
    for parse, argv in ((train.get_arguments, ['--synthetic']),
                        (generate.get_arguments, ['ck']),
                        (evaluate.get_arguments, ev)):
        for bad in ('1.0', '-0.5', 'nan'):
            with pytest.raises(SystemExit):
                parse(argv + ['--preemphasis', bad])
    capsys.readouterr()


def test_checkpoints_carry_the_entry(tmp_path):
    import train
    path = str(tmp_path / 'model.ckpt-7')
    torch.save({'variables': {}, 'step': 7, 'emphasis': {'alpha': 0.97}},
               path)
    assert checkpoint.stored_emphasis(path) == {'alpha': 0.97}
    plain = str(tmp_path / 'model.ckpt-8')
    torch.save({'variables': {}, 'step': 8}, plain)
    assert checkpoint.stored_emphasis(plain) is None
    assert checkpoint.stored_emphasis(str(tmp_path / 'missing')) is None
    # generate.py / evaluate.py: the entry is the default
    assert from_cli(None, checkpoint.stored_emphasis(path)) == Emphasis(0.97)
    assert from_cli(0.0, checkpoint.stored_emphasis(path)) is None
    # train.py: a continued run against its checkpoint
    opened = checkpoint.open_latest(str(tmp_path))
    assert opened.step == 8
    os.remove(plain)
    opened = checkpoint.open_latest(str(tmp_path))
    args = train.get_arguments(['--synthetic'])
    assert train.emphasis_from_flags(args, opened, True) == Emphasis(0.97)
    assert train.emphasis_from_flags(args, None, False) is None
    args = train.get_arguments(['--synthetic', '--preemphasis', '0.9'])
    assert train.emphasis_from_flags(args, opened, False) == Emphasis(0.9)
    with pytest.raises(ValueError, match='0.9.*0.97'):
        train.emphasis_from_flags(args, opened, True)
    # a fresh logdir holds nothing to continue
    assert train.emphasis_from_flags(args, None, True) == Emphasis(0.9)


def test_save_writes_the_entry_only_where_given(tmp_path):
    class Net(object):
        def state_dict(self):
            return {}
    checkpoint.save(Net(), str(tmp_path / 'a'), 3,
                    emphasis=Emphasis(0.97).entry())
    checkpoint.save(Net(), str(tmp_path / 'b'), 3)
    a = torch.load(str(tmp_path / 'a' / 'model.ckpt-3'))
    b = torch.load(str(tmp_path / 'b' / 'model.ckpt-3'))
    assert a['emphasis'] == {'alpha': 0.97} and 'emphasis' not in b


def test_destream_keeps_whole_chunks(monkeypatch):
    """DeStream with a stand-in filter: what it returns is the filter of the
    whole array, fed in growing prefixes; it refilters only from the last
    multiple of the chunk."""
    f = Emphasis(0.9)
    calls = []

    class Host(object):
        def __init__(self, a):
            self.a = a

        def cpu(self):
            return self

        def numpy(self):
            return self.a

    def de(audio, initial=None):
        calls.append((len(audio), None if initial is None
                      else float(initial[0])))
        return Host(f.reference_de(audio, initial=initial))
    monkeypatch.setattr(f, 'de', de)
    monkeypatch.setattr(Emphasis, 'chunk', staticmethod(lambda: 8))
    x = np.random.default_rng(3).uniform(-1, 1, 30).astype(np.float32)
    whole = f.reference_de(x)
    s = DeStream(f)
    for n in (5, 9, 9, 20, 30):
        assert s.feed(x[:n]).tobytes() == whole[:n].tobytes()
    assert [c[0] for c in calls] == [5, 9, 1, 12, 14]
    assert calls[0][1] is None and calls[2][1] == float(whole[7])


def test_entry_points_validate_without_a_device(hip_lib):
    """wn_preemphasis / wn_deemphasis: every check comes before a launch."""
    import ctypes
    buf = (ctypes.c_float * 256)()
    a = ctypes.addressof(buf)
    b = a + 4 * 128
    C = hip_lib.wn_emphasis_chunk()
    assert C > 0 and C % 256 == 0
    pre, de = hip_lib.wn_preemphasis, hip_lib.wn_deemphasis
    assert pre(None, b, 8, 8, 1, 8, None, 0.5, None) == -5
    assert de(a, None, 8, 8, 1, 8, None, None, None, 0.5, None) == -5
    for alpha in (1.0, -0.1, float('nan')):
        assert pre(a, b, 8, 8, 1, 8, None, alpha, None) == -1
        assert de(a, b, 8, 8, 1, 8, None, None, None, alpha, None) == -1
    assert pre(a, b, 7, 8, 1, 8, None, 0.5, None) == -1          # ld < T
    assert de(a, b, 8, 7, 1, 8, None, None, None, 0.5, None) == -1
    assert pre(a, b, 8, 8, 0, 8, None, 0.5, None) == -1
    assert de(a, b, 8, 8, 1, 0, None, None, None, 0.5, None) == -1
    assert pre(a + 2, b, 8, 8, 1, 8, None, 0.5, None) == -3
    assert de(a, b, 8, 8, 1, 8, a + 1, None, None, 0.5, None) == -3
    assert de(a, b, 8, 8, 1, 8, None, a + 2, None, 0.5, None) == -3
    assert de(a, b, 8, 8, 1, 8, None, None, b + 2, 0.5, None) == -3
    # aliasing: never for the pre-emphasis; the de-emphasis in place only
    assert pre(a, a, 8, 8, 2, 8, None, 0.5, None) == -2
    assert pre(a, a + 4 * 4, 8, 8, 2, 8, None, 0.5, None) == -2
    assert de(a, a + 4 * 4, 8, 8, 2, 8, None, None, None, 0.5, None) == -2
    assert de(a, a, 8, 9, 2, 8, None, None, None, 0.5, None) == -2
