"""Local conditioning in fast and batched generation on the GPU: every path
(single workgroup, step kernels, persistent launch, batched) against the
float64 restatement (tests/lc_ref.py), all-zero LC bitwise equal to the model
without LC, causality / alignment of the rows, chunk and batch invariance,
forward priming, the draws and generate.py --lc_fast_generation."""
import os
import sys

import numpy as np
import pytest
import torch

import draw_ref as D
import lc_ref
from util import ROOT

sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

TOL = 1e-5     # the fastgen tests' bar (probabilities)
PATHS = ('single', 'steps', 'persist')


def _model(lc, dilations, S=64, Q=64, biases=True, gc=None, seed=0):
    from wavenet import WaveNetModel
    kw = {}
    if gc:
        kw.update(global_condition_channels=gc, global_condition_cardinality=gc)
    net = WaveNetModel(1, dilations, 2, 32, 32, S, quantization_channels=Q,
                       use_biases=biases, seed=seed,
                       local_condition_channels=lc, **kw)
    g = torch.Generator().manual_seed(seed + 7)
    with torch.no_grad():
        for n, v in net.named_variables():
            if biases and 'bias' in n.split('/')[-1]:
                v.copy_(0.1 * torch.randn(v.shape, generator=g,
                                          dtype=torch.float64).float())
            if lc and n.split('/')[-1].startswith('lc_'):
                # LC weights large enough that the rows matter
                v.copy_(0.3 * torch.randn(v.shape, generator=g,
                                          dtype=torch.float64).float())
    return net


def _path(net, path):
    net.fastgen_multi_cu = path != 'single'
    net.fastgen_persistent = path == 'persist'


def _rows(T, Lc, seed, B=None):
    rng = np.random.default_rng(seed)
    shape = (T, Lc) if B is None else (B, T, Lc)
    return rng.standard_normal(shape).astype(np.float32)


def _softmax(x):
    x = x - x.max(-1, keepdims=True)
    e = np.exp(x)
    return e / e.sum(-1, keepdims=True)


def _ref_probs(net, codes, lc, gc_ids=None):
    """float64 probabilities [B, T, Q] of the codes [B, T] under rows lc."""
    var = lc_ref.model_tree(net)
    lg = lc_ref.logits(var, net.dilations, np.asarray(codes)[None]
                       if np.ndim(codes) == 1 else codes,
                       None if lc is None else (np.asarray(lc)[None]
                                                if np.ndim(lc) == 2 else lc),
                       gc_ids, net.use_biases, net.Q)
    return _softmax(lg)


CASES = [
    # (biases, gc, Lc, dilations, steps, chunk)
    (True, 4, 80, [1, 2, 4, 8, 16, 32, 64, 128, 256, 512], 2000, 7),
    (False, None, 1, [1, 2, 4, 8, 16, 32, 64], 2000, None),
    (True, None, 200, [1, 64, 2, 128, 4, 33], 700, 7),
    (False, 3, 80, [1, 2, 4, 8, 16, 32, 64, 128, 256, 512], 700, None),
]


@pytest.mark.parametrize('case', range(len(CASES)))
def test_every_path_vs_float64(hip_lib, case):
    """Free-running generation (seeded with 3 codes) on every path: the
    probabilities of every step equal the float64 restatement teacher-forced
    on the drawn codes and the same rows; the draws follow draw_ref."""
    biases, gc, Lc, dil, n_steps, chunk = CASES[case]
    net = _model(Lc, dil, biases=biases, gc=gc, seed=case)
    net.fastgen_lc_chunk = chunk
    gid = None if gc is None else [1]
    seed = [5, 9, 2]
    n = n_steps - len(seed) + 1
    lc = _rows(n_steps, Lc, 10 + case)
    outs = {}
    for path in PATHS:
        _path(net, path)
        codes, p = net.generate(n, seed_samples=seed, return_proba_every=1,
                                global_condition=gid, seed=11,
                                local_condition=lc)
        codes, p = codes.cpu().numpy(), p.cpu().numpy()
        assert codes.shape == (n_steps + 1,) and p.shape == (n_steps, net.Q)
        ref = _ref_probs(net, codes[:n_steps], lc, gid)[0]
        err = np.abs(p - ref).max()
        assert err < TOL, (path, err)
        D.check_draws(codes[3:], p[2:], 1.0, 11, np.arange(2, n_steps),
                      what=path)
        outs[path] = (codes, p)
    # batched: B = 1 (shared rows), 37 and 256 streams (own rows)
    for B in (1, 37, 256):
        rows = lc if B == 1 else _rows(n_steps, Lc, 20 + B, B)
        ids = None if gc is None else [b % gc for b in range(B)]
        seeds = [100 + b for b in range(B)]
        codes, p = net.generate_batch(n, seeds, seed_samples=seed,
                                      global_condition=ids,
                                      return_proba_every=1,
                                      local_condition=rows)
        codes, p = codes.cpu().numpy(), p.cpu().numpy()
        for b in sorted({0, B // 2, B - 1}):
            rb = rows if rows.ndim == 2 else rows[b]
            ref = _ref_probs(net, codes[b, :n_steps], rb,
                             None if ids is None else [ids[b]])[0]
            err = np.abs(p[b] - ref).max()
            assert err < TOL, (B, b, err)
            D.check_draws(codes[b, 3:], p[b, 2:], 1.0, seeds[b],
                          np.arange(2, n_steps), what='B %d stream %d' % (B, b))
    # batched B = 1 matches the single-stream generate
    c1, p1 = net.generate_batch(n, [11], seed_samples=seed,
                                global_condition=gid, return_proba_every=1,
                                local_condition=lc)
    codes, p = outs['persist']
    assert np.abs(p1.cpu().numpy()[0] - p).max() < TOL


def test_teacher_forced_vs_float64(hip_lib):
    """Teacher-forced through 600 given codes (no draw), every path."""
    net = _model(80, [1, 2, 4, 8, 16, 32, 64, 128, 256, 512], gc=4, seed=3)
    net.fastgen_lc_chunk = 7
    codes = np.random.default_rng(1).integers(0, net.Q, 600).astype(np.int32)
    lc = _rows(599, 80, 2)
    ref = _ref_probs(net, codes[:599], lc, [2])[0]
    for path in PATHS:
        _path(net, path)
        out, p = net.generate(0, seed_samples=codes, return_proba_every=1,
                              global_condition=[2], local_condition=lc)
        assert np.array_equal(out.cpu().numpy(), codes)
        assert np.abs(p.cpu().numpy() - ref).max() < TOL, path


def _twin(net_lc):
    """The model without LC holding the same weights."""
    from wavenet import WaveNetModel
    kw = {}
    if net_lc.card:
        kw.update(global_condition_channels=net_lc.G,
                  global_condition_cardinality=net_lc.card)
    net = WaveNetModel(1, net_lc.dilations, 2, 32, 32, net_lc.S,
                       quantization_channels=net_lc.Q,
                       use_biases=net_lc.use_biases, **kw)
    src = dict(net_lc.named_variables())
    with torch.no_grad():
        for n, v in net.named_variables():
            v.copy_(src[n])
    return net


@pytest.mark.parametrize('biases,gc', [(True, 4), (False, None)])
def test_zero_lc_bitwise_equals_model_without_lc(hip_lib, biases, gc):
    net = _model(80, [1, 2, 4, 8, 16, 32, 64, 128, 256, 512], biases=biases,
                 gc=gc, seed=5)
    net.fastgen_lc_chunk = 7
    plain = _twin(net)
    gid = None if gc is None else [3]
    z = np.zeros((899, 80), np.float32)
    for path in PATHS:
        _path(net, path)
        _path(plain, path)
        a, pa = net.generate(897, seed_samples=[1, 2, 3], return_proba_every=1,
                             global_condition=gid, seed=4, local_condition=z)
        b, pb = plain.generate(897, seed_samples=[1, 2, 3],
                               return_proba_every=1, global_condition=gid,
                               seed=4)
        assert torch.equal(a, b) and torch.equal(pa, pb), path
    ids = None if gc is None else [1, 2, 3]
    a, pa = net.generate_batch(500, [1, 2, 3], return_proba_every=1,
                               global_condition=ids,
                               local_condition=np.zeros((3, 500, 80)))
    b, pb = plain.generate_batch(500, [1, 2, 3], return_proba_every=1,
                                 global_condition=ids)
    assert torch.equal(a, b) and torch.equal(pa, pb)


def test_causality_and_alignment(hip_lib):
    """Changing row p leaves the probabilities of the steps before p bitwise
    unchanged and changes step p's (the row beside input p conditions the
    prediction of p + 1)."""
    net = _model(8, [1, 2, 4, 8, 16, 32], seed=7)
    net.fastgen_lc_chunk = 5
    codes = np.random.default_rng(3).integers(0, net.Q, 300).astype(np.int32)
    lc = _rows(299, 8, 4)
    for path in PATHS + ('batch',):
        def probs(rows):
            if path == 'batch':
                return net.generate_batch(0, [0], seed_samples=codes,
                                          return_proba_every=1,
                                          local_condition=rows)[1][0]
            _path(net, path)
            return net.generate(0, seed_samples=codes, return_proba_every=1,
                                local_condition=rows)[1]
        base = probs(lc)
        for p in (0, 137, 298):
            mod = lc.copy()
            mod[p] += 1.0
            q = probs(mod)
            assert torch.equal(base[:p], q[:p]), (path, p)
            assert not torch.equal(base[p], q[p]), (path, p)


def test_chunk_invariance_and_continuation(hip_lib):
    net = _model(80, [1, 2, 4, 8, 16, 32, 64, 128, 256, 512], gc=4, seed=9)
    lc = _rows(1200, 80, 6)
    for path in PATHS:
        _path(net, path)
        res = []
        for chunk in (7, None):
            net.fastgen_lc_chunk = chunk
            res.append(net.generate(1200, return_proba_every=1,
                                    global_condition=[1], seed=3,
                                    local_condition=lc))
        assert torch.equal(res[0][0], res[1][0]), path
        assert torch.equal(res[0][1], res[1][1]), path
        # generate(a) then continue_generation(b) on the following rows
        net.fastgen_lc_chunk = 7
        whole = net.generate(1200, global_condition=[1], seed=3,
                             local_condition=lc)
        a = net.generate(500, global_condition=[1], seed=3,
                         local_condition=lc[:500])
        b = net.continue_generation(700, int(a[-1]), global_condition=[1],
                                    seed=3, local_condition=lc[500:])
        assert torch.equal(torch.cat([a, b]), whole), path
    rows = _rows(1200, 80, 7, B=5)
    ids, seeds = [0, 1, 2, 3, 0], [5, 6, 7, 8, 9]
    res = []
    for chunk in (7, None):
        net.fastgen_lc_chunk = chunk
        res.append(net.generate_batch(1200, seeds, global_condition=ids,
                                      return_proba_every=1,
                                      local_condition=rows))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])
    net.fastgen_lc_chunk = 7
    a = net.generate_batch(500, seeds, global_condition=ids,
                           local_condition=rows[:, :500])
    b = net.continue_generation_batch(700, a[:, -1].cpu().numpy(), seeds,
                                      global_condition=ids,
                                      local_condition=rows[:, 500:])
    assert torch.equal(torch.cat([a, b], 1), res[1][0])


def test_batch_invariance(hip_lib):
    """Stream k of B = 37 (own rows, GC id, seed) equals that stream alone,
    bit for bit; permuting the streams permutes the outputs."""
    net = _model(80, [1, 2, 4, 8, 16, 32, 64, 128], gc=5, seed=11)
    net.fastgen_lc_chunk = 7
    B = 37
    rows = _rows(400, 80, 8, B=B)
    ids = [b % 5 for b in range(B)]
    seeds = [1000 + b for b in range(B)]
    codes, p = net.generate_batch(400, seeds, global_condition=ids,
                                  return_proba_every=1, local_condition=rows)
    for k in (0, 13, 36):
        c1, p1 = net.generate_batch(400, [seeds[k]], global_condition=[ids[k]],
                                    return_proba_every=1,
                                    local_condition=rows[k:k + 1])
        assert torch.equal(c1[0], codes[k]) and torch.equal(p1[0], p[k])
    perm = np.random.default_rng(2).permutation(B)
    c2, p2 = net.generate_batch(400, [seeds[i] for i in perm],
                                global_condition=[ids[i] for i in perm],
                                return_proba_every=1,
                                local_condition=rows[perm])
    assert torch.equal(c2, codes[torch.from_numpy(perm)])
    assert torch.equal(p2, p[torch.from_numpy(perm)])


def test_forward_priming_matches_stepping(hip_lib):
    """A seed longer than fastgen_prime_forward_min, primed by the LC forward
    pass, leaves the queues where stepping through it does; two streams with
    equal seed codes and different seed rows are primed apart."""
    net = _model(80, [1, 2, 4, 8, 16, 32, 64, 128], gc=4, seed=13)
    net.fastgen_lc_chunk = 7
    Q, n_seed = net.Q, 150
    assert n_seed - 1 >= net.fastgen_prime_forward_min
    seed = np.random.default_rng(4).integers(0, Q, n_seed).astype(np.int32)
    lc = _rows(n_seed + 99, 80, 9)
    rows = np.stack([lc, lc.copy()])
    rows[1, :n_seed - 1] += 0.5          # other seed rows, same seed codes
    runs = []
    default_min = net.fastgen_prime_forward_min
    for prime_min in (default_min, 10 ** 9):
        net.fastgen_prime_forward_min = prime_min
        try:
            _path(net, 'persist')
            a = net.generate(100, seed_samples=seed, global_condition=[2],
                             seed=1, local_condition=lc)
            more = net.continue_generation(50, int(a[-1]),
                                           global_condition=[2], seed=1,
                                           local_condition=_rows(50, 80, 1))
            bc = net.generate_batch(100, [1, 1], seed_samples=seed,
                                    global_condition=[2, 2],
                                    local_condition=rows)
            bm, bp = net.continue_generation_batch(
                50, bc[:, -1].cpu().numpy(), [1, 1], global_condition=[2, 2],
                return_proba_every=1, local_condition=_rows(50, 80, 1))
        finally:
            net.fastgen_prime_forward_min = default_min
        runs.append((a.cpu().numpy(), more.cpu().numpy(), bc.cpu().numpy(),
                     bm.cpu().numpy(), bp.cpu().numpy()))
    r0, r1 = runs
    assert np.array_equal(r0[0][:n_seed], seed)
    for x, y in zip(r0[:4], r1[:4]):
        assert np.array_equal(x, y)
    assert np.abs(r0[4] - r1[4]).max() < TOL
    # the two streams: same seed codes and draw seed, different seed rows
    assert not np.array_equal(r0[4][0], r0[4][1])


def test_peek_and_incremental(hip_lib):
    """predict_proba_incremental with its row equals generate's probabilities;
    a push=False peek does not advance the queues."""
    net = _model(8, [1, 2, 4, 8], seed=15)
    codes = np.random.default_rng(5).integers(0, net.Q, 40).astype(np.int32)
    lc = _rows(40, 8, 5)
    _path(net, 'single')       # (the path predict_proba_incremental runs)
    _, ref = net.generate(0, seed_samples=np.append(codes, 0),
                          return_proba_every=1, local_condition=lc)
    net.prime_generator([], local_condition=np.zeros((0, 8)))
    for t in range(40):
        peek = net.predict_proba_incremental([codes[t]], push=False,
                                             local_condition=lc[t])
        p = net.predict_proba_incremental([codes[t]], local_condition=lc[t])
        assert torch.equal(peek, p)
        assert torch.equal(p, ref[t])


def test_default_stack_16000_samples_vs_float64(hip_lib):
    """The default stack (wavenet_params.json) with Lc = 80 on the persistent
    path: 16000 free-running samples, every step's probabilities equal the
    float64 restatement teacher-forced on the drawn codes."""
    import json
    prm = json.load(open(os.path.join(ROOT, 'wavenet_params.json')))
    net = _model(80, prm['dilations'], S=prm['skip_channels'],
                 Q=prm['quantization_channels'], biases=True, seed=17)
    _path(net, 'persist')
    lc = _rows(16000, 80, 12)
    codes, p = net.generate(16000, return_proba_every=1, seed=2,
                            local_condition=lc)
    codes, p = codes.cpu().numpy(), p.cpu().numpy()
    ref = _ref_probs(net, codes[:16000], lc)[0]
    assert np.abs(p - ref).max() < TOL
    D.check_draws(codes[1:], p, 1.0, 2, np.arange(16000), what='16000')


def test_cli_lc_fast_generation(hip_lib, tmp_path):
    """generate.py --lc_path ... --lc_fast_generation true writes
    1 + hop * frames codes equal to the API call's; so with --save_every and
    with --clips 3."""
    import generate
    import json
    net = _model(3, [1, 2, 4, 8, 16, 32], S=64, Q=256, seed=19)
    ckpt = str(tmp_path / 'model.ckpt-1')
    torch.save({'variables': net.state_dict()}, ckpt)
    params = str(tmp_path / 'params.json')
    json.dump({"filter_width": 2, "sample_rate": 16000,
               "dilations": [1, 2, 4, 8, 16, 32], "residual_channels": 32,
               "dilation_channels": 32, "quantization_channels": 256,
               "skip_channels": 64, "use_biases": True, "scalar_input": False,
               "initial_filter_width": 32, "residual_postproc": False},
              open(params, 'w'))
    feats = _rows(25, 3, 13)
    fpath = str(tmp_path / 'f.npy')
    np.save(fpath, feats)
    hop = 4
    first = np.random.default_rng(7).integers(256, size=(1,)).tolist()
    lc_full = np.zeros((1 + 100, 3), np.float32)
    lc_full[1:] = np.repeat(feats, hop, axis=0)
    want = net.generate(100, seed_samples=first, seed=7,
                        local_condition=lc_full[:100]).cpu().numpy()
    wantb = net.generate_batch(100, [7, 8, 9], seed_samples=first,
                               local_condition=lc_full[:100]).cpu().numpy()
    for extra, expect in (([], want), (['--save_every', '30'], want),
                          (['--clips', '3'], wantb)):
        logdir = tmp_path / ('log%d' % len(os.listdir(tmp_path)))
        rc = generate.main([ckpt, '--wavenet_params', params, '--lc_path',
                            fpath, '--lc_hop', str(hop),
                            '--lc_fast_generation', 'true', '--seed', '7',
                            '--logdir', str(logdir)] + extra)
        assert rc == 0
        out = [os.path.join(d, f) for d, _, fs in os.walk(str(logdir))
               for f in fs if f == 'generated_codes.npy']
        got = np.load(out[0])
        assert got.shape[-1] == 1 + hop * 25
        assert np.array_equal(got, expect), extra


def test_lc_call_is_the_plain_call_chunk_by_chunk(hip_lib, monkeypatch):
    """The library calls of an LC call in ONE chunk are those of the plain
    call on the same path, in order, plus the ring fills and the _lc suffix;
    in chunks of 7 the chain weights are still packed once, the step kernels
    finish once, and every chunk is one persistent launch."""
    from wavenet import _lib
    net = _model(80, [1, 2, 4, 8, 1, 2, 4, 8])
    plain = _twin(net)
    net.fastgen_graph_steps = plain.fastgen_graph_steps = 4
    seed, n = [4, 7, 1], 25
    n_steps = len(seed) - 1 + n
    lc = _rows(n_steps, 80, 31)
    lib = _lib.load()
    names, launches = [], []
    real_call = _lib.call

    def call(name, *args):
        names.append(name)
        return real_call(name, *args)
    monkeypatch.setattr(_lib, 'call', call)
    for entry in ('wn_fastgen_persist', 'wn_fastgen_persist_lc'):
        def launch(*args, entry=entry, real=getattr(lib, entry)):
            code = real(*args)
            names.append(entry)
            launches.append(code)
            return code
        monkeypatch.setattr(lib, entry, launch)

    def trace(model, path, **kw):
        _path(model, path)
        del names[:], launches[:]
        model.generate(n, seed_samples=seed, seed=6, **kw)
        return list(names), list(launches)
    for path in PATHS:
        net.fastgen_lc_chunk = n_steps + 13
        want, ran = trace(plain, path)
        got, ran_lc = trace(net, path, local_condition=lc)
        assert ran == ran_lc == ([0] if path == 'persist' else []), path
        got = [s[:-3] if s.endswith('_lc') else s
               for s in got if s != 'wn_fastgen_lc_bias']
        assert got == want, path
        net.fastgen_lc_chunk = 7
        got, ran_lc = trace(net, path, local_condition=lc)
        # (the single-workgroup kernel needs no packed weights)
        assert got.count('wn_fastgen_pack') == int(path != 'single'), path
        assert got.count('wn_fastgen_finish') == int(path == 'steps'), path
        assert ran_lc == ([0] * -(-n_steps // 7) if path == 'persist'
                          else []), path


def test_persistent_lc_launches_run_and_fall_back(hip_lib, monkeypatch):
    """Every chunk of an LC call on the persistent path is one
    wn_fastgen_persist_lc launch that runs; an expired hand-over wait in the
    third launch restores the state and the call finishes on the _lc step
    kernels from that chunk: the codes of the uninterrupted run and of the
    step kernels, the probabilities within TOL of both."""
    from wavenet import _lib
    dil = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512]
    a = _model(80, dil, gc=4, seed=21)
    b = _model(80, dil, gc=4, seed=21)
    for net, path in ((a, 'persist'), (b, 'steps')):
        net.fastgen_lc_chunk = 7
        _path(net, path)
    lib = _lib.load()
    real = lib.wn_fastgen_persist_lc
    calls = []

    def recording(*args):
        code = real(*args)
        calls.append(code)
        return code
    monkeypatch.setattr(lib, 'wn_fastgen_persist_lc', recording)
    lc = _rows(300, 80, 3)
    kw = dict(seed_samples=[1, 2, 3], return_proba_every=1,
              global_condition=[1], seed=9, local_condition=lc)
    c0, p0 = a.generate(298, **kw)
    assert calls == [0] * 43                    # ceil(300 / 7) launches ran

    def failing(*args):
        # the real launch runs, then reports what an expired wait reports
        code = real(*args)
        calls.append(code)
        if len(calls) == 3:
            torch.cuda.synchronize()
            a._gen['fgp_sync'][12] = 1
        return code
    calls.clear()
    monkeypatch.setattr(lib, 'wn_fastgen_persist_lc', failing)
    with pytest.warns(UserWarning, match='state restored'):
        c1, p1 = a.generate(298, **kw)
    assert calls == [0, 0, 0] and a._gen_launch_failed['persist']
    c2, p2 = b.generate(298, **kw)
    assert torch.equal(c1, c0) and torch.equal(c1, c2)
    assert (p1 - p0).abs().max().item() < TOL
    assert (p1 - p2).abs().max().item() < TOL
    # steps before the failed chunk are the persistent launches' own
    assert torch.equal(p1[:14], p0[:14])
