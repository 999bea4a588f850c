"""The log-mel front end on the device (csrc/wn_features.hip through
wavenet/features.py) against the float64 oracle tests/mel_ref.py, its bitwise
properties, and the model-level interface that feeds local conditioning."""
import numpy as np
import pytest
import torch

import lc_ref
import lc_up_ref
import masked_ref
import mel_ref

pytestmark = pytest.mark.gpu

# The tolerance (mel_ref.MEL_TOL = MEL_TOL_FACTOR x MEL_F32_ERR = 4 x 9.2e-6):
# 4 x the largest absolute error against the float64 oracle of the float32
# numpy restatement of the rule over the shapes (a) - (c), measured on the CPU
# and written down in tests/mel_ref.py.  A float32 sum in another order
# legitimately differs by about as much; the factor leaves room for the MFMA's
# K order.  Each shape is held to 4 x its OWN restatement error as well
# (MEL_F32_ERR_BY_SHAPE), which for the small shapes asks about 20 x more.
MEL_F32_ERR = mel_ref.MEL_F32_ERR
MEL_TOL_FACTOR = mel_ref.MEL_TOL_FACTOR
MEL_TOL = mel_ref.MEL_TOL


def _spec(name, **over):
    from wavenet import features
    kw = dict(mel_ref.SHAPES[name], **over)
    return features.MelSpec(kw.pop('sample_rate'), **kw)


_ORACLE = {}


def _case(name):
    """(audio float32 [B][T], lengths, oracle [B][F][n_mels]) -- computed
    once, shared, never written to."""
    if name not in _ORACLE:
        x, lengths = mel_ref.make_audio(name)
        ref = mel_ref.logmel_batch(x, lengths, **mel_ref.SHAPES[name])
        ref.setflags(write=False)
        _ORACLE[name] = (x, lengths, ref)
    return _ORACLE[name]


def _real_frames(name):
    x, lengths, _ = _case(name)
    hop = mel_ref.SHAPES[name]['hop']
    return [-(-(x.shape[1] if lengths is None else lengths[b]) // hop)
            for b in range(x.shape[0])]


@pytest.mark.parametrize('name', ['a', 'b', 'c'])
def test_matches_float64_oracle(hip_lib, name):
    x, lengths, ref = _case(name)
    kw = mel_ref.SHAPES[name]
    # no compared value sits at the floor
    for b, nf in enumerate(_real_frames(name)):
        n = x.shape[1] if lengths is None else lengths[b]
        assert mel_ref.mel_energy(x[b, :n], **kw).min() > 1e-6
    got = _spec(name)(x, lengths).cpu().numpy()
    assert got.shape == ref.shape and got.dtype == np.float32
    err = np.abs(got - ref).max()
    own = MEL_TOL_FACTOR * mel_ref.MEL_F32_ERR_BY_SHAPE[name]
    print('shape (%s): max abs error %.3g (bound %.3g, the shape\'s own %.3g)'
          % (name, err, MEL_TOL, own))
    assert err <= MEL_TOL
    assert err <= own


def test_samples_read_from_memory_match_the_staged_ones(hip_lib):
    """A hop too large for the tile's samples to be staged in LDS (n_fft 2048,
    hop 1024: 33792 floats) reads them from memory: the same rule."""
    kw = dict(sample_rate=16000, n_fft=2048, hop=1024, win_length=2048,
              n_mels=20)
    rng = np.random.default_rng(5)
    x = rng.uniform(-0.1, 0.1, (2, 5000)).astype(np.float32)
    lengths = (5000, 1500)
    ref = mel_ref.logmel_batch(x, lengths, **kw)
    got = _spec('c', **{k: v for k, v in kw.items() if k != 'sample_rate'})(
        x, lengths).cpu().numpy()
    assert np.abs(got - ref).max() <= MEL_TOL


def test_silence_sits_at_the_floor(hip_lib):
    spec = _spec('a', floor=1e-5)
    got = spec(np.zeros((2, 50), np.float32), [50, 20]).cpu().numpy()
    want = np.zeros((2, 4, 10), np.float32)
    want[0, :] = np.log(np.float32(1e-5))
    want[1, :2] = np.log(np.float32(1e-5))
    # (a float32 log in the log domain: the parity bound)
    assert np.abs(got - want).max() <= MEL_TOL
    assert np.array_equal(got[1, 2:], want[1, 2:])


@pytest.mark.parametrize('name', ['a', 'c'])
def test_clip_in_a_batch_equals_the_clip_alone(hip_lib, name):
    x, lengths, _ = _case(name)
    spec = _spec(name)
    both = spec(x, lengths)
    for b in range(x.shape[0]):
        n = x.shape[1] if lengths is None else lengths[b]
        alone = spec(x[b], None if lengths is None else [n])
        assert torch.equal(alone, both[b]), b
        # ... and cut to its length: the same frames (F differs)
        short = spec(x[b, :n])
        assert torch.equal(short, both[b, :short.shape[0]]), b


def test_garbage_behind_the_length_changes_nothing(hip_lib):
    x, lengths, _ = _case('a')
    spec = _spec('a')
    clean = spec(x, lengths)
    dirty = x.copy()
    for b, n in enumerate(lengths):
        dirty[b, n:] = np.nan if b % 2 else 1e30
    assert torch.equal(spec(dirty, lengths), clean)


def test_frames_behind_the_length_are_zero(hip_lib):
    x, lengths, _ = _case('a')
    out = _spec('a')(x, lengths)
    for b, nf in enumerate(_real_frames('a')):
        assert int(torch.count_nonzero(out[b, nf:])) == 0
        assert float(out[b, :nf].abs().min()) > 0
    # a second tile that holds no real frame at all
    xb = _case('b')[0]
    out = _spec('b')(xb, [24 * 30])
    assert out.shape[1] == 34
    assert int(torch.count_nonzero(out[0, 30:])) == 0


@pytest.mark.parametrize('name', ['a', 'b', 'c'])
def test_two_calls_give_identical_bits(hip_lib, name):
    x, lengths, _ = _case(name)
    spec = _spec(name)
    assert torch.equal(spec(x, lengths), spec(x, lengths))


def test_frame_bits_do_not_depend_on_the_tile_position(hip_lib):
    """Shifting a clip by whole hops shifts its interior frames (the ones whose
    window lies inside both clips), bit for bit: another row of the tile,
    another tile."""
    kw = mel_ref.SHAPES['b']
    x = _case('b')[0][0]
    spec = _spec('b')
    hop, k = kw['hop'], 5
    a = spec(x)
    b = spec(x[k * hop:].copy())
    lo = -(-kw['n_fft'] // hop)
    assert torch.equal(a[k + lo:-lo], b[lo:a.shape[0] - k - lo])


# ---- every kernel shape and edge --------------------------------------------
# The shapes (d) - (i) of tests/mel_ref.py and the pairs either side of the
# staging limit.  Each is held to MEL_TOL_FACTOR x its OWN yardstick
# (mel_ref.MEL_F32_MEASURED: two float32 summation orders and one float32 ulp of
# the largest output, measured on the CPU against the float64 oracle and
# written down there); no bound here comes from the kernel's output.
NEW = list(mel_ref.NEW_SHAPES)
LIMIT = ['gm', 'gp', 'ks', 'km']


def _n(x, lengths, b):
    return x.shape[1] if lengths is None else lengths[b]


def _staged(n_fft, hop):
    """include/wavenet_hip.h, wn_melspec: a tile's 31 hop + n_fft samples,
    one pad float after every `hop` of them at an even hop, and one more float,
    are staged on chip when they fit 16384 floats; else read from memory."""
    total = 31 * hop + n_fft
    pads = (total - 1) // hop if hop % 2 == 0 else 0
    return total + pads + 1 <= 16384


def _check_against_oracle(name, got):
    """Shape, dtype, the (printed) error on the real frames against the shape's
    own bound, exact zeros behind them."""
    x, lengths, ref = _case(name)
    kw = mel_ref.SHAPES[name]
    for b in range(x.shape[0]):
        # no compared value sits at the floor
        assert mel_ref.mel_energy(x[b, :_n(x, lengths, b)], **kw).min() > 1e-6
    assert got.shape == ref.shape and got.dtype == np.float32
    err = np.abs(got - ref).max()
    tol = mel_ref.shape_tol(name)
    print('shape (%s): max abs error %.3g (bound %.3g = 4 x %.3g)'
          % (name, err, tol, mel_ref.MEL_YARDSTICK_BY_SHAPE[name]))
    for b, nf in enumerate(_real_frames(name)):
        assert not got[b, nf:].view(np.uint32).any(), b
        assert np.abs(got[b, :nf]).min() > 0
    assert err <= tol


def test_the_new_shapes_take_the_paths_they_are_named_for():
    paths = {n: _staged(mel_ref.SHAPES[n]['n_fft'], mel_ref.SHAPES[n]['hop'])
             for n in NEW + LIMIT}
    assert paths == dict(d=True, e=True, f=True, g=True, h=False, i=True,
                         gm=False, gp=True, ks=True, km=False)
    # 64 KiB of basis ring, 8 n_fft bytes of window table and the staged
    # floats: (g) is the largest launch at an odd hop, 'gp' (one hop less, with
    # its pad floats) the largest there is -- no allowed setting asks for more
    # on-chip memory
    def floats(n_fft, hop):
        total = 31 * hop + n_fft
        return total + ((total - 1) // hop if hop % 2 == 0 else 0) + 1
    most = max((65536 + 8 * n_fft + 4 * floats(n_fft, hop), n_fft, hop)
               for n_fft in range(64, 2049, 64) for hop in range(1, n_fft + 1)
               if _staged(n_fft, hop))
    assert most == (147296, 2048, 460) and floats(2048, 460) == 16344
    assert 65536 + 8 * 2048 + 4 * floats(2048, 461) == 147280
    assert floats(2048, 462) == 16406 and floats(1024, 494) == 16372


@pytest.mark.parametrize('name', NEW + ['gp'])
def test_matches_float64_oracle_at_every_kernel_shape(hip_lib, name):
    x, lengths, _ = _case(name)
    _check_against_oracle(name, _spec(name)(x, lengths).cpu().numpy())


@pytest.mark.parametrize('staged,memory', mel_ref.LIMIT_PAIRS)
def test_either_side_of_the_staging_limit_is_the_same_rule(hip_lib, staged,
                                                           memory):
    """One hop apart on the same audio, the samples staged on chip and read
    from memory: both meet the float64 oracle within their own bounds."""
    a, b = mel_ref.SHAPES[staged], mel_ref.SHAPES[memory]
    assert {k: v for k, v in a.items() if k != 'hop'} == \
        {k: v for k, v in b.items() if k != 'hop'}
    assert _staged(a['n_fft'], a['hop']) and not _staged(b['n_fft'], b['hop'])
    assert np.array_equal(_case(staged)[0], _case(memory)[0])
    for name in (staged, memory):
        x, lengths, _ = _case(name)
        _check_against_oracle(name, _spec(name)(x, lengths).cpu().numpy())


@pytest.mark.parametrize('name', ['e', 'f', 'h'])
def test_clip_in_a_batch_equals_the_clip_alone_at_the_edges(hip_lib, name):
    """An odd hop with a one-sample clip, a clip that ends on the tile
    boundary, the memory path."""
    x, lengths, _ = _case(name)
    spec = _spec(name)
    both = spec(x, lengths)
    for b in range(x.shape[0]):
        n = lengths[b]
        alone = spec(x[b], [n])
        assert torch.equal(alone, both[b]), b
        short = spec(x[b, :n])
        assert short.shape[0] == -(-n // spec.hop)
        assert torch.equal(short, both[b, :short.shape[0]]), b


@pytest.mark.parametrize('name', ['e', 'h'])
def test_garbage_behind_the_length_changes_nothing_on_either_path(hip_lib,
                                                                  name):
    x, lengths, _ = _case(name)
    spec = _spec(name)
    clean = spec(x, lengths)
    dirty = x.copy()
    for b, n in enumerate(lengths):          # (a whole clip has no tail)
        dirty[b, n::2] = np.nan
        dirty[b, n + 1::2] = 1e30
    assert np.isnan(dirty).any() and (dirty == np.float32(1e30)).any()
    got = spec(dirty, lengths)
    assert not bool(torch.isnan(got).any())
    assert torch.equal(got, clean)


@pytest.mark.parametrize('name', NEW + LIMIT)
def test_two_calls_give_identical_bits_at_every_kernel_shape(hip_lib, name):
    x, lengths, _ = _case(name)
    spec = _spec(name)
    assert torch.equal(spec(x, lengths), spec(x, lengths))


@pytest.mark.parametrize('name,T', [('e', 25 * 40 + 3), ('h', 462 * 40 + 5)])
def test_frame_bits_do_not_depend_on_the_tile_position_odd_hop_and_memory(
        hip_lib, name, T):
    """As for (b): at an odd hop (no pad slots) and on the memory path.  The
    clip has 41 frames; shifted by 5 hops, the interior frames 32 .. of the
    second tile become frames 27 .. of the first."""
    kw = mel_ref.SHAPES[name]
    x = mel_ref.signal(31, kw['sample_rate'], 1, T)[0]
    spec = _spec(name)
    hop, k = kw['hop'], 5
    a = spec(x)
    b = spec(x[k * hop:].copy())
    lo = -(-kw['n_fft'] // hop)
    assert a.shape[0] == 41 and b.shape[0] == 36 and k + lo < 32 < 41 - lo
    assert torch.equal(a[k + lo:-lo], b[lo:a.shape[0] - k - lo])
    assert not torch.equal(a[:36], b)            # (the frames did move)


@pytest.mark.parametrize('name', ['e', 'h'])
def test_row_stride_and_a_base_off_by_four_bytes(hip_lib, name):
    """The entry itself with ld = T + 3, NaN in the three gap columns, and an
    audio base that is 4-byte but not 16-byte aligned: the bits of the
    contiguous call, on the staged and on the memory path."""
    from wavenet import _lib
    x, lengths, _ = _case(name)
    spec = _spec(name)
    want = spec(x, lengths)
    B, T = x.shape
    ld = T + 3
    flat = torch.full((B * ld + 1,), float('nan'), dtype=torch.float32,
                      device='cuda')
    view = flat[1:].view(B, ld)
    view[:, :T] = torch.from_numpy(x).cuda()
    assert view.data_ptr() % 16 == 4 and view.stride() == (ld, 1)
    assert bool(torch.isnan(view[:, T:]).all()) and bool(torch.isnan(flat[0]))
    win, basis, melw = spec.device_tables(view.device)
    nd = torch.tensor(lengths, dtype=torch.int32, device='cuda')
    F = spec.num_frames(T)
    out = torch.full((B, F, spec.n_mels), float('nan'), dtype=torch.float32,
                     device='cuda')
    _lib.call('wn_melspec', _lib.ptr(view), ld, B, T, _lib.ptr(nd),
              _lib.ptr(win), _lib.ptr(basis), _lib.ptr(melw), spec.n_fft,
              spec.hop, spec.n_bins, spec.n_mels, spec.floor, _lib.ptr(out),
              _lib.stream())
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    # whole clips through the stride: the gap columns sit right behind them
    out.fill_(float('nan'))
    _lib.call('wn_melspec', _lib.ptr(view), ld, B, T, None,
              _lib.ptr(win), _lib.ptr(basis), _lib.ptr(melw), spec.n_fft,
              spec.hop, spec.n_bins, spec.n_mels, spec.floor, _lib.ptr(out),
              _lib.stream())
    torch.cuda.synchronize()
    assert torch.equal(out, spec(x))


def test_silence_sits_at_the_floor_on_the_memory_path(hip_lib):
    """(h): read from memory, four mel fragments, the scalar epilogue."""
    spec = _spec('h', floor=1e-5)
    hop, T, lengths = 462, 15251, [15251, 700]
    got = spec(np.zeros((2, T), np.float32), lengths).cpu().numpy()
    assert got.shape == (2, 34, 97)
    want = np.zeros((2, 34, 97), np.float32)
    want[0, :] = np.log(np.float32(1e-5))
    want[1, :2] = np.log(np.float32(1e-5))
    assert np.abs(got - want).max() <= MEL_TOL
    assert not got[1, 2:].view(np.uint32).any()


# ---- the model-level interface ---------------------------------------------
DIL = [1, 2, 4, 8, 1, 2, 4, 8]


def _model(B, Lc, scales, seed=3):
    from wavenet import WaveNetModel
    kw = {}
    if scales is not None:
        kw['local_condition_upsample_scales'] = tuple(scales)
    return WaveNetModel(B, DIL, 2, 32, 32, 64, quantization_channels=64,
                        use_biases=True, seed=seed,
                        local_condition_channels=Lc, **kw)


def _lc_spec(**over):
    from wavenet import features
    kw = dict(n_fft=64, hop=16, n_mels=8)
    kw.update(over)
    return features.MelSpec(8000, **kw)


def _audio(B, T, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(T)
    x = rng.uniform(-0.1, 0.1, (B, T)) + 0.4 * np.sin(0.3 * t)[None, :]
    return x.astype(np.float32)


def test_local_condition_from_audio(hip_lib):
    B, T, lengths = 2, 70, [70, 37]
    audio = _audio(B, T, 1)
    spec = _lc_spec()
    frames = spec(audio, lengths)
    rep = _model(B, 8, None)
    rows = rep.local_condition_from_audio(spec, audio, lengths)
    assert rows.shape == (B, T, 8) and rows.is_cuda
    idx = torch.arange(T, device=rows.device) // 16
    assert torch.equal(rows, frames[:, idx])
    one = rep.local_condition_from_audio(spec, audio[0])
    assert one.shape == (T, 8) and torch.equal(one, rows[0])
    up = _model(B, 8, (4, 4))
    fr = up.local_condition_from_audio(spec, audio, lengths)
    assert torch.equal(fr, frames)
    with pytest.raises(ValueError):
        up.local_condition_from_audio(_lc_spec(n_mels=9), audio)
    with pytest.raises(ValueError):
        up.local_condition_from_audio(_lc_spec(hop=8), audio)
    with pytest.raises(ValueError):
        rep.local_condition_from_audio(_lc_spec(n_mels=9), audio)
    with pytest.raises(ValueError):
        up.local_condition_from_audio(spec, audio, [70, 71])


def test_loss_on_features_from_audio(hip_lib):
    """TINY-sized LC model, Lc 8, hop 16 = 4 x 4: the loss on the front end's
    frames is bitwise the loss on the same frames copied through the host,
    and agrees with the float64 LC oracle fed the float64 mel oracle."""
    B, T, scales, lengths = 3, 100, (4, 4), [100, 41, 77]
    net = _model(B, 8, scales)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for n, v in net.named_variables():
            last = n.split('/')[-1]
            if '/lc_upsample/' in n:
                v.copy_(0.6 * torch.randn(v.shape, generator=g))
            elif 'bias' in last:
                v.copy_(0.1 * torch.randn(v.shape, generator=g))
            elif last.startswith('lc_'):
                v.copy_(0.05 * torch.randn(v.shape, generator=g))
    audio = _audio(B, T, 2)
    spec = _lc_spec()
    a = net.loss(audio, local_condition_batch=net.local_condition_from_audio(
        spec, audio, lengths), local_condition_offset=0, lengths=lengths)
    torch.cuda.synchronize()
    masks = lc_ref.device_relu_masks(net, B, T)
    host = spec(audio, lengths).cpu().numpy()
    b = net.loss(audio, local_condition_batch=host, local_condition_offset=0,
                 lengths=lengths)
    assert float(a) == float(b)
    codes = net.encode(audio).cpu().numpy()
    var = lc_ref.model_tree(net)
    kw = dict(sample_rate=8000, n_fft=64, hop=16, win_length=64, n_mels=8)
    per = [lc_up_ref.loss_and_grads(
        var, DIL, codes[b_:b_ + 1, :n],
        mel_ref.logmel(audio[b_, :n], **kw)[None], [0], scales,
        use_biases=True, quantization_channels=64,
        relu_masks=masked_ref.clip_masks(masks, b_, n))
        for b_, n in enumerate(lengths)]
    ref_loss, _ = masked_ref.assemble(per, lengths)
    print('loss %.8f oracle %.8f' % (float(a), ref_loss))
    assert abs(float(a) - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
