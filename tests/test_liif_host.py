"""CPU: the LIIF decoder's oracle (tests/liif_oracle.py) pinned against the reference's own liif_interpolate
(tests/golden/make_golden_liif.py), the argument validation of the four entry points without a device, and the host side
of LIIFTriPlaneVoxGO: constructor errors and accepted options, state_dict keys, kwargs."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden

import liif_oracle as LO

CASES = [(agg, cell, ens) for agg in ('concat', 'sum') for cell in (True, False) for ens in (True, False)]
INTERP = ('interp_xy', 'interp_yz', 'interp_zx')


def fixture_nets(z, cell, C, dtype=torch.float64):
    """The fixture's three Interp_MLPs, loaded by their reference names with strict=True, as one module."""
    from directvoxgo_amd.liif import InterpMLP
    holder = torch.nn.Module()
    for net in INTERP:
        setattr(holder, net, InterpMLP(C + (4 if cell else 2), C, width=8, depth=3))
    prefix = f'c{int(cell)}_sd_'
    holder.load_state_dict({k[len(prefix):]: torch.from_numpy(v) for k, v in z.items() if k.startswith(prefix)}, strict=True)
    return holder.to(dtype).eval()


@pytest.mark.parametrize('agg, cell, ens', CASES)
def test_oracle_reproduces_the_reference_decoder(agg, cell, ens):
    """The tri-plane fixture test's standing tolerances: values rtol 1e-5 / atol 1e-6, gradients (planes, Interp_MLP
    parameters) rtol 1e-4 / atol 1e-6.  The MLPs run in float64 on the float32 oracle's rows and weights."""
    z = load_golden('liif')
    C = z['plane_xy'].shape[1]
    nets = fixture_nets(z, cell, C)
    planes = {k: torch.from_numpy(z['plane_' + k]).double().requires_grad_() for k in LO.KEYS}
    val = LO.decode(planes, {'xy': nets.interp_xy, 'yz': nets.interp_yz}, z['xyz'], z['xyz_min'], z['xyz_max'],
                    z['world_size'], cell, ens, agg)
    p = f'{agg}_c{int(cell)}_e{int(ens)}_'
    assert val.shape == z[p + 'out'].shape == (400, 3 * C if agg == 'concat' else C)
    err = np.abs(val.detach().numpy() - z[p + 'out'])
    print('worst |err|', err.max(), 'at values up to', np.abs(z[p + 'out']).max())
    np.testing.assert_allclose(val.detach().numpy(), z[p + 'out'], rtol=1e-5, atol=1e-6)
    val.backward(torch.from_numpy(z[agg + '_gout']).double())
    for k in LO.KEYS:
        np.testing.assert_allclose(planes[k].grad.numpy(), z[f'{p}gplane_{k}'], rtol=1e-4, atol=1e-6)
    for name, q in nets.named_parameters():
        if name.startswith('interp_zx.'):
            assert q.grad is None and f'{p}g_{name}' not in z           # built, stored, never used: no gradient
        else:
            np.testing.assert_allclose(q.grad.numpy(), z[f'{p}g_{name}'], rtol=1e-4, atol=1e-6)


def test_fixture_covers_the_edge_cases():
    """Shifted positions that the clamp moves, on both ends; every shift of some sample on one texel and four different
    texels for another; a plane axis of size 1; E = 1 among the cases; a non-cubic world_size."""
    z = load_golden('liif')
    ws = z['world_size']
    assert len(set(ws.tolist())) > 1 and z['plane_zx'].shape[3] == 1
    for key in LO.KEYS:
        H, W = z['plane_' + key].shape[2:]
        au, av, ia, ib = LO.TABLE[key]
        u = LO._norm(z['xyz'][:, au], z['xyz_min'][au], z['xyz_max'][au])
        shifted = u + (np.float32(1) / np.float32(ws[ia]) + np.float32(1e-6))
        assert (shifted > LO.HI).any() and (u - np.float32(1) / np.float32(ws[ia]) < LO.LO).any()
        row, col, rel0, rel1, wgt, _ = LO.geometry(key, H, W, z['xyz'], z['xyz_min'], z['xyz_max'], ws, True)
        distinct = np.array([len(set(zip(row[:, m], col[:, m]))) for m in range(row.shape[1])])
        assert distinct.min() == 1 and distinct.max() == (4 if W > 1 else 2)
        np.testing.assert_allclose(wgt.sum(0), 1, rtol=1e-6)
        one = LO.geometry(key, H, W, z['xyz'], z['xyz_min'], z['xyz_max'], ws, False)
        assert one[0].shape[0] == 1 and (one[4] == 1).all()
    assert any(k.endswith('_e0_out') for k in z) and any(k.endswith('_e1_out') for k in z)


def test_nearest_rounds_half_to_even():
    """index 2.5 -> 2, 3.5 -> 4 (F.grid_sample 'nearest' uses nearbyint), against torch on the CPU."""
    import torch.nn.functional as F
    c = np.array([0.0, 1 / 3], np.float32)                  # ((c + 1) * 6 - 1) / 2 = 2.5, 3.5
    assert LO.near(c, 6).tolist() == [2, 4]
    plane = torch.arange(6, dtype=torch.float32).reshape(1, 1, 1, 6)
    grid = torch.stack([torch.from_numpy(c), torch.zeros(2)], -1).reshape(1, 1, 2, 2)
    assert F.grid_sample(plane, grid, mode='nearest', align_corners=False).flatten().tolist() == [2.0, 4.0]


# ---------------------------------------------------------------------------------------------- entry points
@pytest.fixture(scope='module')
def lib():
    from directvoxgo_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


ONE = ctypes.c_void_p(16)         # any non-null value: rejected before it could be dereferenced, or never reached
PTRS = LO.KEYS + ('xyz', 'mn', 'mx', 'io', 'io2')


def _geo(lib, name, M=8, C=4, sizes=((6, 7), (3, 9), (8, 2)), null=(), run=0, ws=(13, 13, 9), cell=1, ens=1):
    P = lambda k: None if k in null else ONE         # noqa: E731
    planes = []
    for k, (H, W) in zip(LO.KEYS, sizes):
        planes += [P(k), H, W, 1, W * C, C]
    tail = [C, P('xyz'), P('mn'), P('mx'), M, *ws, cell, ens]
    if name == 'dvgo_liif_gather':
        return getattr(lib, name)(*planes, *tail, P('io'), P('io2'), None)
    return getattr(lib, name)(P('io'), *planes, *tail, run, None)


@pytest.mark.parametrize('name', ['dvgo_liif_gather', 'dvgo_liif_scatter'])
def test_gather_and_scatter_validate_before_any_launch(lib, name):
    ptrs = PTRS if name == 'dvgo_liif_gather' else PTRS[:-1]
    assert _geo(lib, name, M=0) == 0 and _geo(lib, name, C=0) == 0                  # no-ops, pointers not looked at
    assert _geo(lib, name, M=0, null=PTRS) == 0
    assert _geo(lib, name, M=-1) == -1 and _geo(lib, name, C=-1) == -1
    for k in ptrs:
        assert _geo(lib, name, null=(k,)) == -1, k
    assert _geo(lib, name, sizes=((6, 7), (0, 9), (8, 2))) == -1                    # a plane axis below 1
    assert _geo(lib, name, sizes=((6, 7), (3, 9), (8, -2))) == -1
    for ws in ((0, 13, 9), (13, -1, 9), (13, 13, 0)):                               # a world extent below 1
        assert _geo(lib, name, ws=ws) == -1
    big = (1 << 31) // (3 * 4 * 8) + 1                                              # M * 3 E D >= 2^31 at C = 4, D = 8, E = 4
    assert _geo(lib, name, M=big) == -2 and _geo(lib, name, M=big - 1, null=('xyz',)) == -1
    assert _geo(lib, name, M=big, ens=0, cell=0, null=('xyz',)) == -1               # E = 1, D = 6: in range again
    assert _geo(lib, name, M=big, C=0) == 0
    if name == 'dvgo_liif_scatter':
        assert _geo(lib, name, run=-1) == -1


@pytest.mark.parametrize('name', ['dvgo_liif_blend_fwd', 'dvgo_liif_blend_bwd'])
def test_blend_validates_before_any_launch(lib, name):
    def call(M=8, C=4, E=4, null=()):
        a, b, c = (None if i in null else ONE for i in range(3))
        return getattr(lib, name)(a, b, C, M, E, 0, c, None)
    assert call(M=0) == 0 and call(C=0) == 0 and call(M=0, null=(0, 1, 2)) == 0
    assert call(M=-1) == -1 and call(C=-1) == -1
    for E in (0, 2, 3, 5, -1):
        assert call(E=E) == -1
    for i in range(3):
        assert call(null=(i,)) == -1
    big = (1 << 31) // (3 * 4 * 4) + 1
    assert call(M=big) == -2 and call(M=big, E=1, null=(0,)) == -1 and call(M=big, C=0) == 0


def test_ops_reject_cpu_tensors_and_bad_arguments():
    from directvoxgo_amd.ops import liif_blend, liif_gather
    planes = {k: torch.zeros(1, 4, 5, 6) for k in LO.KEYS}
    xyz, mn, mx = torch.zeros(7, 3), -torch.ones(3), torch.ones(3)
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        liif_gather(planes, xyz, mn, mx, (8, 8, 8))
    with pytest.raises(ValueError, match='three'):
        liif_gather([planes['xy']] * 2, xyz, mn, mx, (8, 8, 8))
    with pytest.raises(ValueError, match='aggregation'):
        liif_blend(torch.zeros(3, 4, 7, 4), torch.zeros(3, 4, 7), 'mean')
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        liif_blend(torch.zeros(3, 4, 7, 4), torch.zeros(3, 4, 7))


# ---------------------------------------------------------------------------------------------- model, host side
BASE = dict(num_voxels=10 * 12 * 14, num_voxels_base=16 ** 3, alpha_init=1e-2, fast_color_thres=1e-4)
BOX = ([-1.0, -1.2, -1.4], [1.0, 1.2, 1.4])
# configs/nerf/tri_lego.py: fine_model_and_render without the encoder's keys (name, pretrained_state_dict, map_depth)
TRI_LEGO = dict(implicit_voxel_feat=True, feat_unfold=False, cell_decode=True, local_ensemble=True, rgbnet_dim=32, posbase_pe=0,
                rgbnet_depth=3, global_cell_decode=False, no_voxel_feat=False, cat_posemb=False, interp_width=128,
                interp_depth=5, tri_aggregation='sum', liif=True, feat_pe=0, feat_fourier=False)


def _model(**kw):
    from directvoxgo_amd.liif import LIIFTriPlaneVoxGO
    return LIIFTriPlaneVoxGO(*BOX, **{**BASE, **kw})


def _interp_keys(depth):
    layers = ['model.0'] + [f'model.{i}.0' for i in range(2, depth)] + [f'model.{depth}']
    return {f'{net}.{layer}.{wb}' for net in INTERP for layer in layers for wb in ('weight', 'bias')}


def test_tri_lego_options_state_dict_and_kwargs():
    from directvoxgo_amd.checkpoint import model_kwargs_of
    from directvoxgo_amd.triplane import TriPlaneVoxGO
    m = _model(**TRI_LEGO)
    assert isinstance(m, TriPlaneVoxGO) and not hasattr(m, 'k0') and m.cell_decode and m.local_ensemble
    base = {'xyz_min', 'xyz_max', 'density', 'viewfreq', 'planes.xy', 'planes.yz', 'planes.zx', 'rgbnet.0.weight',
            'rgbnet.0.bias', 'rgbnet.2.0.weight', 'rgbnet.2.0.bias', 'rgbnet.3.weight', 'rgbnet.3.bias', 'mask_cache.mask',
            'mask_cache.xyz2ijk_scale', 'mask_cache.xyz2ijk_shift'}
    assert set(m.state_dict()) == base | _interp_keys(5)
    assert m.interp_xy.model[0].in_features == 32 + 4 and m.interp_xy.model[5].out_features == 32
    assert m.interp_xy.model[2][1].p == 0.1 and m.rgbnet[0].in_features == 32 - 3 + 27          # 'sum': feat_dim = rgbnet_dim
    kw = m.get_kwargs()
    for k in ('implicit_voxel_feat', 'liif', 'cell_decode', 'local_ensemble'):
        assert kw[k] is True
    assert kw['interp_width'] == 128 and kw['interp_depth'] == 5 and kw['interp_dropout'] == 0.1 and kw['tri_aggregation'] == 'sum'
    m2 = type(m)(**model_kwargs_of({'model_kwargs': kw}))
    assert set(m2.state_dict()) == set(m.state_dict()) and m2.get_kwargs().keys() == kw.keys()
    assert all(m2.state_dict()[k].shape == v.shape for k, v in m.state_dict().items())


def test_accepted_options():
    m = _model(rgbnet_dim=4, cell_decode=False, local_ensemble=False, interp_width=16, interp_depth=2, interp_dropout=0.0)
    assert m.interp_yz.model[0].in_features == 4 + 2 and set(m.state_dict()) >= _interp_keys(2)
    assert m.feat_dim == 12 and m.rgbnet[0].in_features == 12 - 3 + 27 and 'posfreq' not in m.state_dict()
    p = _model(rgbnet_dim=4, posbase_pe=4, cat_posemb=True)                       # lib/tri_dvgo.py:212-223
    assert p.rgbnet[0].in_features == 12 - 3 + 27 + (3 + 3 * 4 * 2) and p.posfreq.tolist() == [1, 2, 4, 8]
    assert p.get_kwargs()['posbase_pe'] == 4 and p.get_kwargs()['cat_posemb'] is True
    q = _model(rgbnet_dim=4, posbase_pe=4)                                        # the buffer alone: nothing reads it
    assert q.rgbnet[0].in_features == 12 - 3 + 27 and 'posfreq' in q.state_dict()
    d = _model(rgbnet_dim=4, rgbnet_direct=True, tri_aggregation='sum')
    assert d.rgbnet[0].in_features == 4 + 27
    assert not m.can_keep_count_on_device() and not m.uses_posenc


def test_fixture_decoders_load_by_their_reference_names():
    z = load_golden('forward_liif')
    m = _model(rgbnet_dim=4, interp_width=16, interp_depth=3, rgbnet_width=64, tri_aggregation='sum')
    sd = {k[len('sum_sd_'):]: torch.from_numpy(v) for k, v in z.items() if k.startswith('sum_sd_')}
    assert set(sd) == {k for k in m.state_dict() if k.startswith(('interp_', 'rgbnet.'))}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and not [k for k in missing if k.startswith(('interp_', 'rgbnet.'))]
    assert torch.equal(m.interp_zx.model[3].bias, sd['interp_zx.model.3.bias'])


@pytest.mark.parametrize('kw, match', [
    (dict(feat_unfold=True), 'feat_unfold'), (dict(liif=False), 'liif=False'), (dict(implicit_voxel_feat=False), 'TriPlaneVoxGO'),
    (dict(global_cell_decode=True), 'global_cell_decode'), (dict(feat_fourier=True), 'feat_fourier'), (dict(feat_pe=4), 'feat_pe'),
    (dict(no_voxel_feat=True), 'no_voxel_feat'), (dict(posbase_pe=5, no_voxel_feat=True), 'no_voxel_feat'),
    (dict(rgbnet_full_implicit=True), 'rgbnet_full_implicit'), (dict(name='edsr-baseline'), 'encoder'),
    (dict(pretrained_state_dict='x.pth'), 'encoder'), (dict(map_depth=5), 'encoder'), (dict(rgbnet_dim=0), 'rgbnet_dim')])
def test_left_out_options_raise_with_their_reason(kw, match):
    with pytest.raises(NotImplementedError, match=match):
        _model(**{'rgbnet_dim': 4, **kw})


def test_left_out_methods_and_data_parallel_raise(monkeypatch):
    import torch.distributed as dist
    from directvoxgo_amd.export import extract_mesh
    from directvoxgo_amd.liif import TRI_LIIF_FINE_TRAIN
    from directvoxgo_amd.train import TrainStep
    m = _model(rgbnet_dim=4)
    with pytest.raises(NotImplementedError, match='extract_mesh'):
        extract_mesh(m)
    with pytest.raises(ValueError, match='interp_depth'):
        _model(rgbnet_dim=4, interp_depth=1)
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_world_size', lambda group=None: 2)
    with pytest.raises(NotImplementedError, match='without k0'):
        TrainStep(m, TRI_LIIF_FINE_TRAIN, dict(near=0.5, far=6.0, bg=1, stepsize=0.5))


def test_optimizer_groups_follow_tri_lego():
    from directvoxgo_amd.liif import TRI_LIIF_FINE_TRAIN
    from directvoxgo_amd.train import create_optimizer_or_freeze_model
    m = _model(rgbnet_dim=4, interp_depth=3)
    opt = create_optimizer_or_freeze_model(m, TRI_LIIF_FINE_TRAIN, global_step=0)
    lr = {id(p): g['lr'] for g in opt.param_groups for p in g['params']}
    for net in INTERP + ('rgbnet',):
        assert all(lr[id(p)] == 5e-4 for p in getattr(m, net).parameters()), net
    assert all(lr[id(p)] == TRI_LIIF_FINE_TRAIN['lrate_planes'] for p in m.planes.values())
    assert lr[id(m.density)] == TRI_LIIF_FINE_TRAIN['lrate_density'] and len(lr) == 1 + 3 + 6 + 3 * 6


@pytest.mark.parametrize('kw', [dict(implicit_voxel_feat=True), dict(liif=True), dict(cell_decode=True), dict(feat_unfold=True),
                                dict(posbase_pe=5, cat_posemb=True)])
def test_the_bilinear_class_still_rejects_the_decoder_options(kw):
    from directvoxgo_amd.triplane import TriPlaneVoxGO
    with pytest.raises(NotImplementedError):
        TriPlaneVoxGO(*BOX, **{**BASE, 'rgbnet_dim': 4, **kw})
