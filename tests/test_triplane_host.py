"""CPU: the tri-plane sampler's oracle (tests/triplane_oracle.py) pinned against the reference's own grid_sampler2D
(tests/golden/make_golden_triplane.py), the argument validation of both entry points without a device, and the host side
of TriPlaneVoxGO: constructor errors, kwargs, state_dict keys, plane sizes."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden

import triplane_oracle as TO

AGGS = ('concat', 'sum')


def _planes(z):
    return {k: z['plane_' + k] for k in TO.KEYS}


@pytest.mark.parametrize('agg', AGGS)
def test_oracle_reproduces_the_reference_sampler(agg):
    """The sampler's standing tolerances (tests/test_gpu_ops.py, grid_sampler fixture): values rtol 1e-5 / atol 1e-6,
    gradients rtol 1e-4 / atol 1e-6; and the reference's float32 output within 5 u A of the oracle (4 products and 4
    additions per plane, in float32, against sums in float64: measured worst ratio 0.63)."""
    z = load_golden('triplane')
    planes = _planes(z)
    val, A = TO.forward(planes, z['xyz'], z['xyz_min'], z['xyz_max'], agg)
    ref = z[agg + '_out']
    assert val.shape == ref.shape
    np.testing.assert_allclose(val, ref, rtol=1e-5, atol=1e-6)
    ratio = np.abs(val - ref) / np.maximum(5 * TO.U * A, 1e-300)
    print('forward worst |err| / (5 u A):', ratio.max())
    assert (np.abs(val - ref) <= 5 * TO.U * A).all()
    grads = TO.backward({k: p.shape[1:] for k, p in planes.items()}, z['xyz'], z['xyz_min'], z['xyz_max'], z[agg + '_gout'], agg)
    for k in TO.KEYS:
        g, Ag, n = grads[k]
        np.testing.assert_allclose(g, z[f'{agg}_gplane_{k}'][0], rtol=1e-4, atol=1e-6)
        assert (g[:, n == 0] == 0).all() and (z[f'{agg}_gplane_{k}'][0][:, n == 0] == 0).all()


def test_fixture_covers_the_edge_cases():
    """Points on the box corners, on texel centres and outside the box: somewhere all four corners are kept, somewhere two
    (one axis out of range: two dropped) and somewhere one (both axes: three dropped)."""
    z = load_golden('triplane')
    dropped = set()
    for k in TO.KEYS:
        _, _, w, ok = TO.corners(k, *z['plane_' + k].shape[2:], z['xyz'], z['xyz_min'], z['xyz_max'])
        dropped |= set((4 - ok.sum(0)).tolist())
        if k == 'xy':
            assert ((w == 1).any(0)).sum() >= 8          # texel centres: one corner carries the whole weight
    assert {0, 2, 3} <= dropped
    assert z['plane_zx'].shape[3] == 1                     # an axis of size 1


def test_axis_table():
    """Plane xy varies only along its rows when the point moves along y, and only along its columns along z, and so on:
    the mapping of include/dvgo_hip.h, checked against the reference expressions on the CPU."""
    import torch.nn.functional as F
    mn, mx = np.array([-1, -1, -1], np.float32), np.array([1, 1, 1], np.float32)
    table = {'xy': (1, 2), 'yz': (0, 1), 'zx': (2, 0)}
    pairs = {'xy': [0, 1], 'yz': [1, 2], 'zx': [2, 0]}
    for key, (ah, aw) in table.items():
        H, W = 4, 5
        rows = np.arange(H, dtype=np.float32)[:, None].repeat(W, 1)[None, None]          # value = row index
        cols = np.arange(W, dtype=np.float32)[None, :].repeat(H, 0)[None, None]
        for axis in range(3):
            xyz = np.zeros((2, 3), np.float32)
            xyz[1, axis] = 0.5
            for plane, follows in ((rows, ah), (cols, aw)):
                planes = {k: np.zeros((1, 1, H, W), np.float32) for k in TO.KEYS}
                planes[key] = plane
                v, _ = TO.forward(planes, xyz, mn, mx, 'sum')
                assert (v[0, 0] != v[1, 0]) == (axis == follows), (key, axis)
                ind = ((torch.from_numpy(xyz).reshape(1, 1, -1, 3) + 1) / 2).flip((-1,)) * 2 - 1
                ref = F.grid_sample(torch.from_numpy(plane), ind[..., pairs[key]], mode='bilinear', align_corners=True)[0, :, 0, :].T
                np.testing.assert_allclose(v, ref.numpy(), atol=1e-6)


# ---------------------------------------------------------------------------------------------- entry points
@pytest.fixture(scope='module')
def lib():
    from directvoxgo_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def _args(lib, name, M=8, C=4, sizes=((6, 7), (3, 9), (8, 2)), null=(), run=0):
    one = ctypes.c_void_p(16)         # any non-null value: rejected before it could be dereferenced, or never reached
    P = lambda k: None if k in null else one         # noqa: E731
    planes = []
    for k, (H, W) in zip(TO.KEYS, sizes):
        planes += [P(k), H, W, 1, W * C, C]
    tail = [C, P('xyz'), P('mn'), P('mx'), M, 0]
    if name == 'dvgo_triplane_fwd':
        return getattr(lib, name)(*planes, *tail, P('io'), None)
    return getattr(lib, name)(P('io'), *planes, *tail, run, None)


@pytest.mark.parametrize('name', ['dvgo_triplane_fwd', 'dvgo_triplane_bwd'])
def test_entry_points_validate_before_any_launch(lib, name):
    assert _args(lib, name, M=0) == 0 and _args(lib, name, C=0) == 0                # no-ops, pointers not looked at
    assert _args(lib, name, M=0, null=TO.KEYS + ('xyz', 'mn', 'mx', 'io')) == 0
    assert _args(lib, name, M=-1) == -1 and _args(lib, name, C=-1) == -1
    for k in TO.KEYS + ('xyz', 'mn', 'mx', 'io'):
        assert _args(lib, name, null=(k,)) == -1, k
    assert _args(lib, name, sizes=((6, 7), (0, 9), (8, 2))) == -1                   # a plane axis below 1
    assert _args(lib, name, sizes=((6, 7), (3, 9), (8, -2))) == -1
    assert _args(lib, name, M=(1 << 31) // 12 + 1) == -2                            # M * 3C >= 2^31
    assert _args(lib, name, M=(1 << 31) // 12 + 1, C=0) == 0
    if name == 'dvgo_triplane_bwd':
        assert _args(lib, name, run=-1) == -1


def test_op_rejects_cpu_tensors_and_bad_arguments():
    from directvoxgo_amd.ops import triplane_sample
    planes = {k: torch.zeros(1, 4, 5, 6) for k in TO.KEYS}
    xyz, mn, mx = torch.zeros(7, 3), -torch.ones(3), torch.ones(3)
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        triplane_sample(planes, xyz, mn, mx)
    with pytest.raises(ValueError, match='aggregation'):
        triplane_sample(planes, xyz, mn, mx, aggregation='mean')
    with pytest.raises(ValueError, match='three'):
        triplane_sample([planes['xy']] * 2, xyz, mn, mx)
    with pytest.raises(RuntimeError, match=r'\[1,C,H,W\]'):
        triplane_sample({**planes, 'xy': torch.zeros(4, 5, 6)}, xyz, mn, mx)


# ---------------------------------------------------------------------------------------------- model, host side
BASE = dict(num_voxels=10 * 12 * 14, num_voxels_base=16 ** 3, alpha_init=1e-2, fast_color_thres=1e-4)
BOX = ([-1.0, -1.2, -1.4], [1.0, 1.2, 1.4])


def _model(**kw):
    from directvoxgo_amd.triplane import TriPlaneVoxGO
    return TriPlaneVoxGO(*BOX, **{**BASE, **kw})


@pytest.mark.parametrize('agg', AGGS)
def test_constructor_state_dict_and_kwargs(agg):
    from directvoxgo_amd.voxel_model import VoxelModel
    m = _model(rgbnet_dim=4, rgbnet_width=64, tri_aggregation=agg)
    assert isinstance(m, VoxelModel) and not hasattr(m, 'k0')
    expect = {'xyz_min', 'xyz_max', 'density', 'viewfreq', 'planes.xy', 'planes.yz', 'planes.zx', 'rgbnet.0.weight',
              'rgbnet.0.bias', 'rgbnet.2.0.weight', 'rgbnet.2.0.bias', 'rgbnet.3.weight', 'rgbnet.3.bias', 'mask_cache.mask',
              'mask_cache.xyz2ijk_scale', 'mask_cache.xyz2ijk_shift'}
    assert set(m.state_dict()) == expect
    assert isinstance(m.planes, torch.nn.ParameterDict) and all(float(p.detach().abs().sum()) == 0 for p in m.planes.values())
    feat = 12 if agg == 'concat' else 4
    assert m.feat_dim == feat and m.rgbnet[0].in_features == feat - 3 + 27          # lib/tri_dvgo.py:212-223
    assert _model(rgbnet_dim=4, rgbnet_direct=True, tri_aggregation=agg).rgbnet[0].in_features == feat + 27
    assert not m.can_keep_count_on_device() and not m.uses_posenc
    kw = m.get_kwargs()
    assert kw['tri_aggregation'] == agg and kw['plane_size'] is None and kw['rgbnet_dim'] == 4
    from directvoxgo_amd.checkpoint import model_kwargs_of
    m2 = type(m)(**model_kwargs_of({'model_kwargs': kw}))
    assert set(m2.state_dict()) == expect and all(m2.state_dict()[k].shape == v.shape for k, v in m.state_dict().items())


def test_plane_sizes_follow_world_size_or_plane_size():
    m = _model(rgbnet_dim=4)
    X, Y, Z = (int(v) for v in m.world_size)
    assert len({X, Y, Z}) == 3
    assert tuple(m.planes['xy'].shape) == (1, 4, Y, Z)          # rows y, columns z
    assert tuple(m.planes['yz'].shape) == (1, 4, X, Y)          # rows x, columns y
    assert tuple(m.planes['zx'].shape) == (1, 4, Z, X)          # rows z, columns x
    assert all(p.stride(1) == 1 for p in m.planes.values())     # channels-last storage
    assert all(p.is_contiguous() for p in _model(rgbnet_dim=4, channels_last=False).planes.values())
    f = _model(rgbnet_dim=4, plane_size=(5, 9))
    assert all(tuple(p.shape) == (1, 4, 5, 9) for p in f.planes.values()) and f.get_kwargs()['plane_size'] == (5, 9)


def test_optimizer_picks_up_the_planes():
    from directvoxgo_amd.train import create_optimizer_or_freeze_model
    from directvoxgo_amd.triplane import TRI_FINE_TRAIN
    m = _model(rgbnet_dim=4)
    opt = create_optimizer_or_freeze_model(m, TRI_FINE_TRAIN, global_step=0)
    groups = {id(p): g['lr'] for g in opt.param_groups for p in g['params']}
    assert all(groups[id(p)] == TRI_FINE_TRAIN['lrate_planes'] for p in m.planes.values())
    assert groups[id(m.density)] == TRI_FINE_TRAIN['lrate_density'] and len(groups) == 1 + 3 + 6


@pytest.mark.parametrize('kw, match', [
    (dict(implicit_voxel_feat=True), 'implicit_voxel_feat'), (dict(liif=True), 'liif'), (dict(feat_unfold=True), 'feat_unfold'),
    (dict(cell_decode=True), 'cell_decode'), (dict(global_cell_decode=True), 'global_cell_decode'),
    (dict(feat_fourier=True), 'feat_fourier'), (dict(feat_pe=4), 'feat_pe'),
    (dict(posbase_pe=5, cat_posemb=True), 'cat_posemb'), (dict(posbase_pe=5, no_voxel_feat=True), 'no_voxel_feat'),
    (dict(rgbnet_full_implicit=True), 'rgbnet_full_implicit'), (dict(name='edsr-baseline'), 'encoder'),
    (dict(n_resblocks=16), 'encoder'), (dict(rgbnet_dim=0), 'rgbnet_dim')])
def test_out_of_scope_options_raise(kw, match):
    with pytest.raises(NotImplementedError, match=match):
        _model(**{'rgbnet_dim': 4, **kw})


def test_out_of_scope_methods_raise():
    from directvoxgo_amd.export import extract_mesh
    m = _model(rgbnet_dim=4)
    with pytest.raises(NotImplementedError, match='k0'):
        m.k0_total_variation_add_grad(1.0, True)
    with pytest.raises(NotImplementedError, match='extract_mesh'):
        extract_mesh(m)
    with pytest.raises(NotImplementedError, match='encoder'):
        m.encode_feat(None, None)
    with pytest.raises(ValueError, match='tri_aggregation'):
        _model(rgbnet_dim=4, tri_aggregation='mean')


def test_data_parallel_training_raises(monkeypatch):
    import torch.distributed as dist
    from directvoxgo_amd.train import TrainStep
    from directvoxgo_amd.triplane import TRI_FINE_TRAIN
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_world_size', lambda group=None: 2)
    with pytest.raises(NotImplementedError, match='without k0'):
        TrainStep(_model(rgbnet_dim=4), TRI_FINE_TRAIN, dict(near=0.5, far=6.0, bg=1, stepsize=0.5))
