"""Local conditioning in fast generation, host side (no GPU): the keyword,
shape and refusal rules of the fast entry points, raised before any device
work; the chunk plan of the conditioned-bias ring; the new library symbols
and their argument validation; generate.py's --lc_fast_generation."""
import ctypes

import numpy as np
import pytest

from util import ROOT  # noqa: F401  (puts the package on sys.path)


def _net(lc=None, **kw):
    from wavenet import WaveNetModel
    args = dict(batch_size=1, dilations=[1, 2, 4, 8], filter_width=2,
                residual_channels=32, dilation_channels=32, skip_channels=64,
                quantization_channels=256, use_biases=True, device='cpu')
    args.update(kw)
    return WaveNetModel(**args, local_condition_channels=lc)


class _NoDevice(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    """Every check must raise before the fast-generation module is reached."""
    from wavenet import fastgen

    def boom(*a, **k):
        raise _NoDevice()
    # (the batch calls check their rows in _batch_args, whose last check
    # refuses a model without a GPU device)
    for name in ('generate', 'prime', 'continue_generation',
                 'predict_proba_incremental'):
        monkeypatch.setattr(fastgen, name, boom)


def test_local_condition_is_keyword_only():
    from wavenet import WaveNetModel
    import inspect
    for name in ('generate', 'continue_generation', 'prime_generator',
                 'predict_proba_incremental', 'generate_batch',
                 'continue_generation_batch'):
        p = inspect.signature(getattr(WaveNetModel, name)).parameters
        assert p['local_condition'].kind == inspect.Parameter.KEYWORD_ONLY
        assert p['local_condition'].default is None


def test_refusal_without_rows_names_the_keyword(no_device):
    net = _net(lc=4)
    for c in (lambda: net.generate(10), lambda: net.reset_generator(),
              lambda: net.prime_generator([1, 2]),
              lambda: net.continue_generation(4, 3),
              lambda: net.predict_proba_incremental([3]),
              lambda: net.generate_batch(4, [1, 2]),
              lambda: net.continue_generation_batch(4, [1, 2], [1, 2])):
        with pytest.raises(NotImplementedError, match='predict_proba') as e:
            c()
        assert 'local_condition' in str(e.value)
    # reset_generator refuses even with rows at hand: prime_generator([]) resets
    with pytest.raises(NotImplementedError, match='prime_generator'):
        net.reset_generator()


def test_rows_on_a_model_without_lc(no_device):
    net = _net()
    z = np.zeros((3, 4), np.float32)
    for c in (lambda: net.generate(3, local_condition=z),
              lambda: net.continue_generation(3, 1, local_condition=z),
              lambda: net.prime_generator([1, 2, 3], local_condition=z),
              lambda: net.predict_proba_incremental([1], local_condition=z[0]),
              lambda: net.generate_batch(3, [1], local_condition=z),
              lambda: net.continue_generation_batch(3, [1], [1],
                                                    local_condition=z)):
        with pytest.raises(ValueError, match='without local'):
            c()


def test_shapes_checked_before_the_device(no_device):
    net = _net(lc=4)
    bad = [
        # (call, expected shape in the message)
        (lambda z: net.generate(10, local_condition=z), '[10, 4]'),
        (lambda z: net.generate(10, seed_samples=[1, 2, 3],
                                local_condition=z), '[12, 4]'),
        (lambda z: net.continue_generation(5, 3, local_condition=z), '[5, 4]'),
        (lambda z: net.prime_generator([1, 2], local_condition=z), '[2, 4]'),
        (lambda z: net.predict_proba_incremental([3], local_condition=z),
         '[1, 4]'),
        (lambda z: net.generate_batch(4, [1, 2], local_condition=z),
         '[2, 4, 4]'),
        (lambda z: net.continue_generation_batch(4, [1, 2], [1, 2],
                                                 local_condition=z),
         '[2, 4, 4]'),
    ]
    for c, shape in bad:
        with pytest.raises(ValueError, match=r'\[') as e:
            c(np.zeros((7, 3), np.float32))
        assert shape in str(e.value)
    with pytest.raises(ValueError, match='floating point'):
        net.generate(2, local_condition=np.zeros((2, 4), np.int32))
    # shapes that pass reach the fast-generation module (and nothing else)
    ok = [lambda: net.generate(10, seed_samples=[1, 2, 3],
                               local_condition=np.zeros((12, 4))),
          lambda: net.continue_generation(5, 3,
                                          local_condition=np.zeros((5, 4))),
          lambda: net.prime_generator([], local_condition=np.zeros((0, 4))),
          lambda: net.predict_proba_incremental(
              [3], local_condition=np.zeros(4)),
          lambda: net.generate_batch(4, [1, 2],
                                     local_condition=np.zeros((4, 4))),
          lambda: net.generate_batch(4, [1, 2],
                                     local_condition=np.zeros((2, 4, 4))),
          lambda: net.continue_generation_batch(
              4, [1, 2], [1, 2], local_condition=np.zeros((4, 4)))]
    from wavenet import _lib
    for c in ok:
        with pytest.raises((_NoDevice, _lib.WaveNetHipError)):
            c()
    # the stream count is checked before the rows, as without LC
    for seeds in ([], list(range(300))):
        with pytest.raises(ValueError, match='streams'):
            net.generate_batch(4, seeds, local_condition=np.zeros((7, 3)))
        with pytest.raises(ValueError, match='streams'):
            net.continue_generation_batch(4, seeds, seeds,
                                          local_condition=np.zeros((7, 3)))


def test_torch_seed_codes(no_device):
    """Seed codes as a torch tensor: the rows' length is counted from it, and
    a model without LC takes it as before (to the device check)."""
    import torch
    from wavenet import _lib
    net = _net()
    with pytest.raises(_NoDevice):
        net.generate(3, seed_samples=torch.tensor([1, 2, 3]))
    lcnet = _net(lc=4)
    with pytest.raises(_NoDevice):
        lcnet.generate(3, seed_samples=torch.tensor([1, 2, 3]),
                       local_condition=torch.zeros(5, 4))
    with pytest.raises(ValueError, match=r'\[5, 4\]'):
        lcnet.generate(3, seed_samples=torch.tensor([1, 2, 3]),
                       local_condition=torch.zeros(4, 4))
    with pytest.raises(_lib.WaveNetHipError):
        net.generate_batch(3, [1], seed_samples=torch.tensor([1, 2, 3]))


def test_forward_priming_needs_the_lc_stack_launch(no_device):
    """An LC seed is primed by the forward pass only where that pass carries
    the rows (wn_stack_fwd_lc, as predict_proba); prime_generator refuses
    otherwise, before any device work."""
    net = _net(lc=4)
    assert net._lc_forward_ok(100)
    net.stack_fwd = False
    assert not net._lc_forward_ok(100)
    with pytest.raises(NotImplementedError, match='stack'):
        net.prime_generator([1, 2, 3], local_condition=np.zeros((3, 4)))
    # (no codes: a reset, which needs no forward pass)
    with pytest.raises(_NoDevice):
        net.prime_generator([], local_condition=np.zeros((0, 4)))


def test_wide_lc_models_refused_naming_the_limit(no_device):
    net = _net(lc=4, skip_channels=1024)
    with pytest.raises(NotImplementedError, match='512'):
        net.generate(2, local_condition=np.zeros((2, 4)))
    net = _net(lc=4, dilations=[1, 2] * 33)
    with pytest.raises(NotImplementedError, match='64 layers'):
        net.generate_batch(2, [1], local_condition=np.zeros((2, 4)))


def test_chunk_plan():
    from wavenet.fastgen import lc_chunk, lc_plan
    # forced chunk, rounded up to the probability stride, at most n_steps
    assert lc_chunk(1000, 4096, forced=7) == 7
    assert lc_chunk(1000, 4096, forced=7, proba_every=3) == 9
    assert lc_chunk(5, 4096, forced=7) == 5
    with pytest.raises(ValueError):
        lc_chunk(10, 4096, forced=0)
    # automatic: the ring budget holds C + 1 rows, C a multiple of the graph
    row = 50 * 256 * 64 * 4               # L = 50, B = 256
    c = lc_chunk(10 ** 6, row, graph_steps=20)
    assert c % 20 == 0 and (c + 1) * row <= 256 << 20 and c >= 20
    assert lc_chunk(10 ** 6, row, graph_steps=200) == 200   # one graph at least
    from wavenet.fastgen import LC_RING_BYTES_ONE
    one = lc_chunk(10 ** 6, 50 * 64 * 4, budget=LC_RING_BYTES_ONE)  # one stream
    assert one == 2600 and (one + 1) * 50 * 64 * 4 <= LC_RING_BYTES_ONE
    # the plan: chunks cover every step once; chunk (a, n) fills rows
    # a .. a + n, so the ring needs R = C + 1 rows and the last chunk's last
    # row is the zero lookahead row n_steps
    for n_steps, C in ((20, 7), (21, 7), (7, 7), (1, 5)):
        plan = lc_plan(n_steps, C)
        steps = [a + i for a, n in plan for i in range(n)]
        assert steps == list(range(n_steps))
        assert all(n <= C for _, n in plan)
        a, n = plan[-1]
        assert a + n == n_steps
        rows = [list(range(a, a + n + 1)) for a, n in plan]
        assert all(len(r) <= C + 1 for r in rows)
    assert lc_plan(0, 7) == []


def test_new_symbols_validate_without_gpu(hip_lib):
    from wavenet import _lib
    for name in ('wn_fastgen_lc_bias', 'wn_fastgen_run_lc', 'wn_fastgen_pre_lc',
                 'wn_fastgen_step_lc', 'wn_fastgen_persist_lc',
                 'wn_fastgen_batch_pre_lc', 'wn_fastgen_batch_step_lc'):
        assert hasattr(hip_lib, name) and name in _lib.SIGNATURES
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    lib = hip_lib
    # ring kernel: NULL, n_rows > R, a shared ring with per-stream rows, B
    assert lib.wn_fastgen_lc_bias(None, 0, 4, a, 2, None, 0, 1, 0, 1, a, 2, 64,
                                  None) == -5
    assert lib.wn_fastgen_lc_bias(a, 0, 4, a, 2, None, 0, 1, 0, 3, a, 2, 64,
                                  None) == -1
    assert lib.wn_fastgen_lc_bias(a, 16, 4, a, 2, None, 0, 2, 0, 1, a, 2, 0,
                                  None) == -1
    assert lib.wn_fastgen_lc_bias(a, 0, 4, a, 2, None, 0, 1, 0, 1, a, 2, 32,
                                  None) == -1
    assert lib.wn_fastgen_lc_bias(a, 0, 4, a, 2, None, 0, 300, 0, 1, a, 2, 64,
                                  None) == -2
    # _lc entry points: a NULL ring, a bad R or stride
    run = lambda ring, R, st: lib.wn_fastgen_run_lc(
        a, a, 0, a, None, a, None, a, None, None, a, 2, 64, 16, a, a, a, 1, 1,
        1.0, 0, None, 1, 0, 1, ring, R, st, None)
    assert run(None, 2, 64) == -5
    assert run(a, 0, 64) == -1
    assert run(a, 2, 7) == -1
    assert lib.wn_fastgen_pre_lc(a, 0, None, a, 2, a, a, a, None, 2, 64,
                                 None) == -5
    assert lib.wn_fastgen_pre_lc(a, 0, None, a, 2, a, a, a, a, 0, 64,
                                 None) == -1
    step = lambda ring, R: lib.wn_fastgen_step_lc(
        a, a, 0, a, None, a, None, a, None, None, a, 2, 64, 16, a, a, a, a,
        None, 0, a, a, a, a, a, a, ring, R, 64, None)
    assert step(None, 2) == -5 and step(a, -1) == -1
    persist = lambda ring, R: lib.wn_fastgen_persist_lc(
        a, a, 0, a, None, a, None, a, None, None, a, 2, 64, 16, a, a, a, a,
        None, 0, a, a, a, a, a, a, a, a, 5, ring, R, 64, None)
    assert persist(None, 2) == -5 and persist(a, 0) == -1
    assert lib.wn_fastgen_batch_pre_lc(a, 0, None, 0, a, 2, 3, a, a, a, None,
                                       2, 64, None) == -5
    assert lib.wn_fastgen_batch_pre_lc(a, 0, None, 0, a, 2, 3, a, a, a, a,
                                       2, 5, None) == -1
    bstep = lambda ring, R: lib.wn_fastgen_batch_step_lc(
        a, a, 0, a, None, a, None, a, None, None, 0, a, 2, 64, 16, 3, a, a, a,
        a, a, a, None, 0, a, a, a, a, a, ring, R, 64, None)
    assert bstep(None, 2) == -5 and bstep(a, 0) == -1


def test_cli_lc_fast_generation_flag():
    import generate
    a = generate.get_arguments(['ckpt', '--lc_path', 'f.npy'])
    assert a.lc_fast_generation is False
    a = generate.get_arguments(['ckpt', '--lc_path', 'f.npy',
                                '--lc_fast_generation', 'true'])
    assert a.lc_fast_generation is True
    a = generate.get_arguments(['ckpt', '--lc_fast_generation', 'False'])
    assert a.lc_fast_generation is False
    with pytest.raises(SystemExit):
        generate.get_arguments(['ckpt', '--lc_fast_generation', 'maybe'])


def test_cli_refusal_names_both_ways(tmp_path, capsys):
    import generate
    np.save(str(tmp_path / 'f.npy'), np.zeros((4, 3), np.float32))
    rc = generate.main([str(tmp_path / 'model.ckpt-1'), '--lc_path',
                        str(tmp_path / 'f.npy')])
    out = capsys.readouterr().out
    assert rc == 1
    assert '--fast_generation false' in out
    assert '--lc_fast_generation true' in out
