"""Batched fast generation without a GPU: argument validation of the
wn_fastgen_batch_* entry points (all return before any launch), generate.py's
--clips / --gc_ids, and the errors WaveNetModel.generate_batch raises before
it touches a device."""
import ctypes
import sys

import numpy as np
import pytest

from util import ROOT, TINY, cfg_with, model_kwargs

sys.path.insert(0, ROOT)
import generate  # noqa: E402

C32 = cfg_with(TINY, residual_channels=32, dilation_channels=32, batch_size=1)


def test_batch_rows_and_state_size(hip_lib):
    assert hip_lib.wn_fastgen_batch_rows(0) == -1
    assert hip_lib.wn_fastgen_batch_rows(-3) == -1
    assert hip_lib.wn_fastgen_batch_rows(257) == -2
    assert [hip_lib.wn_fastgen_batch_rows(b) for b in (1, 32, 33, 37, 256)] == \
        [32, 32, 64, 64, 256]
    dil = np.array([1, 2, 4], np.int32)
    d = dil.ctypes.data
    assert hip_lib.wn_fastgen_batch_state_floats(None, 3, 4) == -5
    assert hip_lib.wn_fastgen_batch_state_floats(d, 0, 4) == -1
    assert hip_lib.wn_fastgen_batch_state_floats(d, 65, 4) == -2
    assert hip_lib.wn_fastgen_batch_state_floats(d, 3, 0) == -1
    assert hip_lib.wn_fastgen_batch_state_floats(d, 3, 257) == -2
    assert hip_lib.wn_fastgen_batch_state_floats(d, 3, 5) == 7 * 32 * 32
    assert hip_lib.wn_fastgen_batch_state_floats(d, 3, 40) == 7 * 64 * 32


def test_batch_entry_points_validate_arguments(hip_lib):
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    lib = hip_lib
    # init
    assert lib.wn_fastgen_batch_init(None, 64, a, a, 4, None) == -5
    assert lib.wn_fastgen_batch_init(a, 64, a, None, 4, None) == -5
    assert lib.wn_fastgen_batch_init(a, 64, a, a, 0, None) == -1
    assert lib.wn_fastgen_batch_init(a, 64, a, a, 257, None) == -2
    assert lib.wn_fastgen_batch_init(a, 0, a, a, 4, None) == -1
    # pre
    assert lib.wn_fastgen_batch_pre(a, 0, None, 0, a, 4, 2, a, None, a, None) == -5
    assert lib.wn_fastgen_batch_pre(a, 0, None, 32, a, 4, 2, a, a, a, None) == -1
    assert lib.wn_fastgen_batch_pre(a, 0, None, 0, a, 65, 2, a, a, a, None) == -2
    assert lib.wn_fastgen_batch_pre(a, 0, None, 64, a, 4, 0, a, a, a, None) == -1
    assert lib.wn_fastgen_batch_pre(a, 0, None, 64, a, 4, 300, a, a, a, None) == -2

    # step: (L, S, Q, B) and one pointer to drop
    def step(L=4, S=64, Q=256, B=2, stride=0, drop=None):
        p = [a] * 32
        if drop is not None:
            p[drop] = None
        return lib.wn_fastgen_batch_step(
            p[0], p[1], 0, p[2], None, p[3], None, p[4], None, None, stride,
            p[5], L, S, Q, B, p[6], p[7], p[8], p[9], p[10], p[11], None, 1,
            p[12], p[13], p[14], p[15], p[16], None)
    for k in range(17):
        assert step(drop=k) == -5, k
    assert step(L=0) == -1
    assert step(S=0) == -1
    assert step(stride=16) == -1
    assert step(B=0) == -1
    assert step(B=257) == -2
    assert step(S=516) == -2
    assert step(Q=516) == -2
    assert step(L=65) == -2

    # single stages: the same checks, plus the stage range
    def stages(first, last, drop=None):
        p = [a] * 32
        if drop is not None:
            p[drop] = None
        return lib.wn_fastgen_batch_stages(
            first, last, p[0], p[1], 0, p[2], None, p[3], None, p[4], None,
            None, 0, p[5], 4, 64, 256, 2, p[6], p[7], p[8], p[9], p[10], p[11],
            None, 1, p[12], p[13], p[14], p[15], p[16], None)
    assert stages(0, 5, drop=3) == -5
    for first, last in ((-1, 2), (0, 6), (3, 3), (4, 2)):
        assert stages(first, last) == -1, (first, last)
    # finish
    assert lib.wn_fastgen_batch_finish(256, 2, None, a, a, a, None, a, None) == -5
    assert lib.wn_fastgen_batch_finish(256, 2, a, a, a, None, None, a, None) == -5
    assert lib.wn_fastgen_batch_finish(0, 2, a, a, a, a, None, a, None) == -1
    assert lib.wn_fastgen_batch_finish(600, 2, a, a, a, a, None, a, None) == -2
    assert lib.wn_fastgen_batch_finish(256, 0, a, a, a, a, None, a, None) == -1
    assert lib.wn_fastgen_batch_finish(256, 257, a, a, a, a, None, a, None) == -2


def test_generate_arguments_clips_and_gc_ids():
    a = generate.get_arguments(['ck'])
    assert a.clips == 1 and a.gc_ids is None
    a = generate.get_arguments(['ck', '--clips', '4'])
    assert a.clips == 4 and a.gc_ids is None
    a = generate.get_arguments(['ck', '--gc_channels', '8', '--gc_cardinality',
                                '10', '--gc_ids', '1,4,7'])
    assert a.clips == 3 and a.gc_ids == [1, 4, 7] and a.gc_id is None
    # one id: the single-clip path with that id
    a = generate.get_arguments(['ck', '--gc_channels', '8', '--gc_cardinality',
                                '10', '--gc_ids', '5'])
    assert a.clips == 1 and a.gc_ids is None and a.gc_id == 5
    a = generate.get_arguments(['ck', '--clips', '2', '--gc_ids', '3,9'])
    assert a.clips == 2 and a.gc_ids == [3, 9]
    with pytest.raises(ValueError):
        generate.get_arguments(['ck', '--clips', '2', '--gc_ids', '1,2,3'])
    with pytest.raises(ValueError):
        generate.get_arguments(['ck', '--clips', '0'])
    with pytest.raises(ValueError):
        generate.get_arguments(['ck', '--gc_id', '1', '--gc_ids', '1,2'])
    with pytest.raises(ValueError):
        generate.get_arguments(['ck', '--clips', '3', '--fast_generation',
                                'false'])


def _cpu_net(cfg, **kw):
    from wavenet import WaveNetModel
    return WaveNetModel(device='cpu', **model_kwargs(cfg_with(cfg, **kw)))


def test_generate_batch_argument_errors(hip_lib):
    net = _cpu_net(C32, global_condition_channels=4,
                   global_condition_cardinality=10)
    with pytest.raises(ValueError, match='same number'):
        net.generate_batch(5, [1, 2], seed_samples=[[1, 2, 3], [4, 5]])
    with pytest.raises(ValueError, match='rows for 3 streams'):
        net.generate_batch(5, [1, 2, 3], seed_samples=[[1, 2], [4, 5]])
    with pytest.raises(ValueError, match='2 ids for 3 streams'):
        net.generate_batch(5, [1, 2, 3], global_condition=[1, 2])
    with pytest.raises(ValueError, match='1 to 256 streams'):
        net.generate_batch(5, list(range(257)))
    with pytest.raises(ValueError, match='1 to 256 streams'):
        net.generate_batch(5, [])
    with pytest.raises(ValueError, match='temperature'):
        net.generate_batch(5, [1, 2], temperature=0.0)
    with pytest.raises(ValueError, match='3 codes for 2 streams'):
        net.continue_generation_batch(5, [1, 2, 3], [1, 2])


# the message points to the path that does run the model: generate() for the
# shapes only the batched kernels lack, predict_proba where no fast generation
# path exists
@pytest.mark.parametrize('kw,what,instead', [
    (dict(residual_channels=64, dilation_channels=64), '32 residual', 'generate()'),
    (dict(filter_width=3), 'filter_width 2', 'predict_proba'),
    (dict(scalar_input=True, initial_filter_width=32), 'one-hot', 'predict_proba'),
    (dict(skip_channels=1024), '512 skip', 'generate()'),
], ids=['wide', 'filter_width', 'scalar_input', 'skip'])
def test_generate_batch_unsupported_models(hip_lib, kw, what, instead):
    net = _cpu_net(C32, **kw)
    for call in (lambda: net.generate_batch(4, [0, 1]),
                 lambda: net.continue_generation_batch(4, [3, 3], [0, 1])):
        with pytest.raises(NotImplementedError, match=what) as e:
            call()
        assert instead in str(e.value)
