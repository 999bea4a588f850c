"""The workspace cache on the host (wavenet/workspace.py): every view carved
out of an owner fits inside the owner's buffers -- for every model kind,
variant word of the stack launches, batch size and pair of lengths, including
the lengths either side of the 16- / 32-row tile boundary -- and the owner
policy of `get`.  device='cpu' models: workspaces are built, nothing runs."""
import itertools

import pytest
import torch

BASE = dict(dilations=[1, 2], filter_width=2, residual_channels=32,
            dilation_channels=32, skip_channels=64, quantization_channels=64,
            use_biases=True)
KINDS = {
    'c32_S512': dict(skip_channels=512, quantization_channels=256),
    'gc': dict(global_condition_channels=4, global_condition_cardinality=5),
    'blocked64': dict(residual_channels=64, dilation_channels=64),
    'k3': dict(filter_width=3),
    'scalar': dict(scalar_input=True, initial_filter_width=32),
    'residual_postproc': dict(residual_postproc=True),
    'lc_rows': dict(local_condition_channels=8),
    'lc_up': dict(local_condition_channels=8,
                  local_condition_upsample_scales=(4, 4)),
    'lc_up_ctx': dict(local_condition_channels=8,
                      local_condition_upsample_scales=(4, 4),
                      local_condition_context=2),
    # mixture-of-logistics heads: Q = 3 * Kp = 12, 36 and 96 logit columns
    'mol_k1': dict(scalar_input=True, output_mixture=1),
    'mol_k10_gc': dict(scalar_input=True, initial_filter_width=32,
                       output_mixture=10, global_condition_channels=4,
                       global_condition_cardinality=5),
    'mol_k32_lc_up': dict(scalar_input=True, initial_filter_width=2,
                          output_mixture=32, local_condition_channels=8,
                          local_condition_upsample_scales=(4, 4),
                          local_condition_context=1),
}
BATCHES = (1, 2, 3, 4, 8)
LENGTHS = (1, 17, 33, 500, 4096, 11000, 16000)
# (rows, waves) of every variant word _lib.stack_variant expresses from these
VARIANTS = list(itertools.product((0, 16, 32), (0, 4, 8)))

_nets = {}


def _net(kind):
    from wavenet import WaveNetModel
    if kind not in _nets:
        kw = dict(BASE, batch_size=1, device='cpu')
        kw.update(KINDS[kind])
        _nets[kind] = WaveNetModel(**kw)
    return _nets[kind]


def _boundary(lib, B, variant):
    """(T_lo, T_hi): the lengths, multiples of 32, one 32-row tile either
    side of where the library goes from 16- to 32-row tiles at batch size B
    (asked of the library: whatever CU count it assumes); () when the variant
    word fixes the rows."""
    if lib.wn_stack_tile_rows(B, 32, variant) == 32 or \
            lib.wn_stack_tile_rows(B, 1 << 22, variant) == 16:
        return ()
    lo, hi = 1, 1 << 17                  # in 32-row tiles: rows(lo) == 16
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if lib.wn_stack_tile_rows(B, 32 * mid, variant) == 16:
            lo = mid
        else:
            hi = mid
    assert lib.wn_stack_tile_rows(B, 32 * lo, variant) == 16
    assert lib.wn_stack_tile_rows(B, 32 * hi, variant) == 32
    return (32 * lo, 32 * hi)


def _tensors(ws):
    return {k: v for k, v in vars(ws).items() if isinstance(v, torch.Tensor)}


def _check_view(view, owner):
    N = view.N
    assert view.capacity != view.N and view.capacity == owner.N
    own = _tensors(owner)
    for name, t in _tensors(view).items():
        o = own.get(name)
        if o is None:
            # the view's own (a buffer the owner lacks): never plane sized
            assert t.numel() < N * 32, (name, tuple(t.shape))
            continue
        assert t.data_ptr() == o.data_ptr(), name
        assert t.dtype == o.dtype and t.numel() <= o.numel(), \
            (name, tuple(t.shape), tuple(o.shape))
    for key, reg in getattr(view, 'region', {}).items():
        o = owner.region[key]
        assert reg.buf.data_ptr() == o.buf.data_ptr(), key
        assert reg.buf.numel() <= o.buf.numel(), key
        assert reg.n <= reg.stride, key
        assert reg.count * reg.stride <= reg.buf.numel(), \
            (key, reg.count, reg.stride, reg.buf.numel())
        if reg.buf.dim() == 3:           # [L][count][stride]: slabs per layer
            assert reg.count <= reg.buf.shape[1], (key, reg.count,
                                                   tuple(reg.buf.shape))


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('kind', sorted(KINDS))
def test_every_view_fits_its_owner(hip_lib, kind, B):
    """For every variant word and owner length: workspace.get carves every
    shorter length, training and forward-only, out of the owner without
    raising; every buffer the view shares starts at the owner's address and
    has no more elements; every slab region lies inside its buffer; a view
    allocates nothing of plane size."""
    from wavenet import workspace
    from wavenet._lib import stack_variant
    net = _net(kind)
    for rows, waves in VARIANTS:
        net.stack_variant = stack_variant(rows=rows, waves=waves)
        v = net._stack_variant_for_launch()
        edge = _boundary(hip_lib, B, v)
        assert len(edge) == (2 if rows == 0 and not net.Lc else 0)
        lengths = sorted(set(LENGTHS + edge))
        for i, T_own in enumerate(lengths[1:], 1):
            net._ws = {}
            owner = workspace.get(net, B, T_own, True)
            assert owner.capacity == owner.N == B * T_own
            for T in lengths[:i]:
                what = (kind, rows, waves, B, T_own, T)
                try:
                    tv = workspace.get(net, B, T, True)
                    fv = workspace.get(net, B, T, False)
                except RuntimeError as e:
                    pytest.fail('%s: %s' % (what, e))
                assert tv.training and not fv.training, what
                assert tv.stack_rows == hip_lib.wn_stack_tile_rows(B, T, v)
                _check_view(tv, owner)
                _check_view(fv, owner)
            owners = [w for w in net._ws.values() if w.capacity == w.N]
            assert owners == [owner]
    net.stack_variant = 0
    net._ws = {}


def test_issue_case_waves4_view_across_the_tile_boundary(hip_lib):
    """A 32-row owner just above the tile boundary and a 16-row view just
    below it, four waves per workgroup: the view's backward stack writes more
    weight-gradient slabs per layer than the owner's own launch."""
    from wavenet import workspace
    from wavenet._lib import stack_variant
    net = _net('c32_S512')
    net.stack_variant = v = stack_variant(waves=4)
    T_lo, T_hi = _boundary(hip_lib, 4, v)
    owner = workspace.get(net, 4, T_hi, True)
    view = workspace.get(net, 4, T_lo, True)
    assert (owner.stack_rows, view.stack_rows) == (32, 16)
    need = hip_lib.wn_stack_bwd_slabs(4, T_lo, v)
    assert need > hip_lib.wn_stack_bwd_slabs(4, T_hi, v)
    assert view.region['layers_stack'].count == need <= owner.lslabs.shape[1]
    _check_view(view, owner)
    net.stack_variant = 0


def _owners(net, training):
    return [w for w in net._ws.values()
            if w.capacity == w.N and w.training == training]


def test_longer_training_length_replaces_the_training_owner_only(hip_lib):
    from wavenet import workspace
    net = _net('gc')
    net._ws = {}
    a = workspace.get(net, 2, 500, True)
    f = workspace.get(net, 2, 700, False)            # forward-only owner
    short = workspace.get(net, 2, 300, True)
    assert short.capacity == a.N and f.capacity == f.N
    b = workspace.get(net, 2, 501, True)             # past the owner
    assert _owners(net, True) == [b] and b.capacity == b.N == 2 * 501
    assert _owners(net, False) == [f]
    # every training workspace of the old owner is gone, the views too
    assert [w for w in net._ws.values() if w.training] == [b]
    assert workspace.get(net, 2, 500, True).capacity == b.N     # now a view
    assert workspace.get(net, 2, 700, False) is f
    net._ws = {}


def test_training_at_another_batch_size_evicts_the_training_owner(hip_lib):
    from wavenet import workspace
    net = _net('gc')
    net._ws = {}
    a = workspace.get(net, 2, 500, True)
    workspace.get(net, 2, 100, True)
    f = workspace.get(net, 2, 600, False)
    b = workspace.get(net, 3, 200, True)             # fewer rows, another B
    assert b.capacity == b.N == 600
    assert _owners(net, True) == [b] and _owners(net, False) == [f]
    assert all(w.B == 3 for w in net._ws.values() if w.training)
    a2 = workspace.get(net, 2, 500, True)
    assert a2 is not a and _owners(net, True) == [a2]
    net._ws = {}


def test_more_than_64_cached_views_collapse_to_the_owners(hip_lib):
    from wavenet import workspace
    net = _net('gc')
    net._ws = {}
    tr = workspace.get(net, 1, 400, True)
    fw = workspace.get(net, 1, 450, False)
    last = None
    for T in range(1, 64):                           # 63 views: 65 entries
        assert len(net._ws) == T + 1
        last = workspace.get(net, 1, T, bool(T % 2))
    assert set(net._ws.values()) == {tr, fw, last}
    assert net._ws[(1, 63, True)] is last
    assert sorted(w.N for w in _owners(net, True) + _owners(net, False)) \
        == [400, 450]
    # and a collapsed view comes back as a view of the same owner
    again = workspace.get(net, 1, 10, False)
    assert again.capacity in (tr.N, fw.N) and again.capacity != again.N
    net._ws = {}


# ---- the workspace test's tail enumeration, on models that run nothing ----
def test_workspace_tails_cover_every_streamed_buffer(hip_lib):
    """tests/test_gpu_guard_workspace.py on device='cpu' models: every kind
    takes the path it is there for, every tensor of the owner is either a
    tail or listed as having none, aliases of one allocation form one tail,
    and the fills are the ones the buffers' roles ask for."""
    import test_gpu_guard_workspace as tgw
    import test_gpu_workspace_sequence as seq
    from wavenet import WaveNetModel, workspace
    from util import cfg_with, model_kwargs
    for name, kind, setup, check in tgw.KINDS:
        for B in (1, 3):
            if hasattr(kind, 'cfg'):
                kw = model_kwargs(cfg_with(kind.cfg, batch_size=B))
            else:                        # LcUpCtx.model's arguments
                kw = dict(batch_size=B, dilations=seq.LC_DIL, filter_width=2,
                          residual_channels=32, dilation_channels=32,
                          skip_channels=64, quantization_channels=kind.Q,
                          use_biases=True,
                          global_condition_channels=kind.gc,
                          global_condition_cardinality=kind.gc,
                          local_condition_channels=seq.LC_CH,
                          local_condition_upsample_scales=seq.LC_SCALES,
                          local_condition_context=seq.LC_CTX)
            net = WaveNetModel(device='cpu', **kw)
            if setup:
                setup(net)
            for T in tgw.T_VIEWS:
                net._ws = {}
                owner = workspace.get(net, B, 2 * T + 37, True)
                views = [workspace.get(net, B, T, True),
                         workspace.get(net, B, T, False)]
                check(net, views[0], net._step_path(views[0], True))
                tails, none = tgw._tails(owner, views)
                seen = set(n for names, _, _ in tails for n in names) | \
                    set(n for group in none for n in group.split('|'))
                assert seen == set(tgw._tensors(owner)), (name, B, T)
                fills = {n: f for names, _, f in tails for n in names}
                for n in ('X', 'Z', 'h1', 'h2', 'logits', 'loss_parts'):
                    assert fills[n] == 'float', (name, n)
                assert fills['q'] == fills['q_tgt'] == 'code'
                assert fills['stack_flags'] == 'write_only'
                if name == 'tiny_gc':
                    assert fills['tilesum'] == fills['tilesum16'] == \
                        fills['tilesum_buf'] == 'float'
                    group = [names for names, _, _ in tails
                             if 'tilesum' in names]
                    assert group == [('tilesum', 'tilesum16', 'tilesum_buf')]
                for names, words, _ in tails:
                    big = max((getattr(owner, n) for n in names),
                              key=lambda t: t.numel())
                    used = big.numel() - words.numel()
                    assert 0 < used < big.numel(), names
                    for v in views:
                        t = getattr(v, names[0], None)
                        assert t is None or t.numel() <= used, names
