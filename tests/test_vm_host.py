"""CPU: the vector-matrix sampler's oracle (tests/vm_oracle.py) against a float64 torch restatement, the build and typing
of the two entry points, their argument validation without a device, and the host side of VMTriPlaneVoxGO."""
import ctypes

import numpy as np
import pytest
import torch

import vm_oracle as VO

SIZES = {'xy': (5, 7), 'yz': (6, 4), 'zx': (3, 9)}
LINES = {'xy': 6, 'yz': 1, 'zx': 9}
MN, MX = np.array([-1.0, -0.8, -0.6], np.float32), np.array([0.9, 1.1, 0.7], np.float32)


def test_oracle_agrees_with_the_torch_restatement():
    """500 random points inside and up to two cells (of the coarsest axis, 3 nodes: the box's own extent) outside the box:
    the oracle (float32 coordinates and weights, float64 sums) against six float64 F.grid_sample, product and cat, at the
    sampler's standing tolerances, values rtol 1e-5 / atol 1e-6."""
    rng = np.random.default_rng(11)
    R = 5
    planes = {k: rng.standard_normal((1, R, *hw)).astype(np.float32) for k, hw in SIZES.items()}
    lines = {k: rng.standard_normal((1, R, n, 1)).astype(np.float32) for k, n in LINES.items()}
    xyz = (MN + (MX - MN) * (rng.random((500, 3)) * 3.0 - 1.0)).astype(np.float32)
    val, A = VO.forward(planes, lines, xyz, MN, MX)
    assert val.shape == A.shape == (500, 3 * R) and (A >= np.abs(val) - 1e-12).all()
    t64 = lambda d: {k: torch.from_numpy(v).double() for k, v in d.items()}          # noqa: E731
    ref = VO.torch_restatement(t64(planes), t64(lines), torch.from_numpy(xyz).double(), torch.from_numpy(MN).double(),
                               torch.from_numpy(MX).double()).numpy()
    inside = ((xyz >= MN) & (xyz <= MX)).all(1)
    assert 10 < inside.sum() < 490 and (val[~inside] == 0).any() and (val[~inside] != 0).any()
    print('worst |oracle - torch| / (1e-6 + 1e-5 |torch|):', float((np.abs(val - ref) / (1e-6 + 1e-5 * np.abs(ref))).max()))
    np.testing.assert_allclose(val, ref, rtol=1e-5, atol=1e-6)
    # the float32 restatement of the line is the oracle's line value to 3 u A (two products, one addition)
    for k in VO.KEYS:
        lv, la = VO._line_parts(k, lines[k][0, :, :, 0].astype(np.float64), xyz, MN, MX)
        assert (np.abs(VO.line32(k, lines[k], xyz, MN, MX) - lv) <= 3 * VO.U * la).all()


# ---------------------------------------------------------------------------------------------- build, typing, validation
def test_build_and_typing():
    from directvoxgo_amd import _lib, build
    assert 'vm.hip' in build.SOURCES
    build.build(verbose=False)
    with open(_lib.HEADER_PATH) as f:
        decl = _lib.declarations(f.read())
    P, i, q = _lib._Pointer, ctypes.c_int, ctypes.c_int64
    geom = [P, i, i, q, q, q] * 3 + [P, i, q, q] * 3
    assert decl['dvgo_vm_fwd'] == (ctypes.c_int, geom + [i, P, P, P, q, P, P])
    assert decl['dvgo_vm_bwd'] == (ctypes.c_int, [P] + geom + [P] * 6 + [i, P, P, P, q, i, i, P])
    lib = _lib.lib()
    assert lib.dvgo_vm_fwd.argtypes == decl['dvgo_vm_fwd'][1] and lib.dvgo_vm_bwd.argtypes == decl['dvgo_vm_bwd'][1]
    assert _lib.ABI_VERSION == lib.dvgo_abi_version() == 11


@pytest.fixture(scope='module')
def lib():
    from directvoxgo_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


POINTERS = ('xy', 'yz', 'zx', 'xy_line', 'yz_line', 'zx_line', 'xyz', 'mn', 'mx', 'io')
GRADS = ('g_xy', 'g_yz', 'g_zx', 'gl_xy', 'gl_yz', 'gl_zx')


def _call(lib, name, M=8, R=4, sizes=((6, 7), (3, 9), (8, 2)), lines=(5, 1, 9), null=(), run=0, mode=0):
    one = ctypes.c_void_p(16)         # any non-null value: rejected before it could be dereferenced, or never reached
    P = lambda k: None if k in null else one         # noqa: E731
    geom = []
    for k, (H, W) in zip(VO.KEYS, sizes):
        geom += [P(k), H, W, 1, W * R, R]
    for k, N in zip(VO.KEYS, lines):
        geom += [P(k + '_line'), N, 1, R]
    tail = [R, P('xyz'), P('mn'), P('mx'), M]
    if name == 'dvgo_vm_fwd':
        return lib.dvgo_vm_fwd(*geom, *tail, P('io'), None)
    return lib.dvgo_vm_bwd(P('io'), *geom, *[P(k) for k in GRADS], *tail, run, mode, None)


@pytest.mark.parametrize('name', ['dvgo_vm_fwd', 'dvgo_vm_bwd'])
def test_entry_points_validate_before_any_launch(lib, name):
    every = POINTERS + (GRADS if name == 'dvgo_vm_bwd' else ())
    assert _call(lib, name, M=0) == 0 and _call(lib, name, R=0) == 0                # no-ops
    assert _call(lib, name, M=0, null=every) == 0 and _call(lib, name, R=0, null=every) == 0   # ... that touch no pointer
    assert _call(lib, name, M=-1) == -1 and _call(lib, name, R=-1) == -1
    for k in every:
        assert _call(lib, name, null=(k,)) == -1, k                                  # each pointer is looked at
    assert _call(lib, name, sizes=((6, 7), (0, 9), (8, 2))) == -1                   # a plane axis below 1
    assert _call(lib, name, sizes=((6, 7), (3, 9), (8, -2))) == -1
    assert _call(lib, name, lines=(5, 0, 9)) == -1 and _call(lib, name, lines=(5, 1, -3)) == -1   # a line length below 1
    assert _call(lib, name, M=0, lines=(5, 0, 9)) == -1                             # sizes are judged before the no-op
    assert _call(lib, name, M=(1 << 31) // 12 + 1) == -2                            # M * 3R >= 2^31
    assert _call(lib, name, M=(1 << 31) // 12 + 1, R=0) == 0


def test_bwd_validates_run_and_mode(lib):
    name = 'dvgo_vm_bwd'
    assert _call(lib, name, run=-1) == -1
    assert _call(lib, name, mode=-1) == -1 and _call(lib, name, mode=3) == -1       # an unknown mode
    assert _call(lib, name, M=0, mode=3) == -1 and _call(lib, name, M=0, run=-1) == -1
    # mode 2's table is (N_xy + N_yz + N_zx) * R floats: 64 KB is 16384 of them.  One entry more is refused, on the size
    # alone (the pointers are all valid-looking here and the launch range is not exceeded).
    assert _call(lib, name, M=4, R=4, lines=(2048, 2048, 1), mode=2) == -1          # 4097 * 4 * 4 B = 64 KB + 16 B
    assert _call(lib, name, M=4, R=16, lines=(1024, 1, 1), mode=2) == -1            # 1026 * 16 * 4 B
    assert _call(lib, name, M=0, R=4, lines=(2048, 2048, 1), mode=2) == 0           # nothing to do comes first
    from directvoxgo_amd import _lib
    with pytest.raises(RuntimeError, match='invalid argument'):               # the typed call turns the code into an error
        _lib.call('dvgo_vm_bwd', None, *([None, 1, 1, 1, 1, 1] * 3), *([None, 1, 1, 1] * 3), *([None] * 6), 4, None, None, None, 8,
                  0, 0, None)


def test_ops_reject_cpu_tensors_and_bad_arguments():
    from directvoxgo_amd.ops import vm_sample
    planes = {k: torch.zeros(1, 4, 5, 6) for k in VO.KEYS}
    lines = {k: torch.zeros(1, 4, 7, 1) for k in VO.KEYS}
    xyz, mn, mx = torch.zeros(7, 3), -torch.ones(3), torch.ones(3)
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        vm_sample(planes, lines, xyz, mn, mx)
    with pytest.raises(ValueError, match='three'):
        vm_sample(planes, [lines['xy']] * 2, xyz, mn, mx)
    with pytest.raises(RuntimeError, match=r'\[1,R,N,1\]'):
        vm_sample(planes, {**lines, 'yz': torch.zeros(1, 4, 7, 2)}, xyz, mn, mx)


# ---------------------------------------------------------------------------------------------- model, host side
BASE = dict(num_voxels=10 * 12 * 14, num_voxels_base=16 ** 3, alpha_init=1e-2, fast_color_thres=1e-4)
BOX = ([-1.0, -1.2, -1.4], [1.0, 1.2, 1.4])


def _model(**kw):
    from directvoxgo_amd.vm import VMTriPlaneVoxGO
    return VMTriPlaneVoxGO(*BOX, **{**BASE, **kw})


def test_constructor_kwargs_and_state_dict_round_trip():
    from directvoxgo_amd.checkpoint import model_kwargs_of
    from directvoxgo_amd.triplane import TriPlaneVoxGO
    from directvoxgo_amd.voxel_model import VoxelModel
    m = _model(n_comp=8, rgbnet_dim=6, rgbnet_width=64)
    assert isinstance(m, TriPlaneVoxGO) and isinstance(m, VoxelModel) and not hasattr(m, 'k0')
    expect = {'xyz_min', 'xyz_max', 'density', 'viewfreq', 'planes.xy', 'planes.yz', 'planes.zx', 'lines.xy', 'lines.yz',
              'lines.zx', 'basis', 'rgbnet.0.weight', 'rgbnet.0.bias', 'rgbnet.2.0.weight', 'rgbnet.2.0.bias', 'rgbnet.3.weight',
              'rgbnet.3.bias', 'mask_cache.mask', 'mask_cache.xyz2ijk_scale', 'mask_cache.xyz2ijk_shift'}
    assert set(m.state_dict()) == expect
    assert m.feat_dim == 6 and m.rgbnet[0].in_features == 6 - 3 + 27 and tuple(m.basis.shape) == (24, 6)
    assert _model(n_comp=8, rgbnet_dim=6, rgbnet_direct=True).rgbnet[0].in_features == 6 + 27
    assert _model().n_comp == 16 and _model().line_size is None                     # the defaults
    kw = m.get_kwargs()
    assert kw['n_comp'] == 8 and kw['line_size'] is None and kw['plane_size'] is None and kw['rgbnet_dim'] == 6
    assert 'tri_aggregation' not in kw
    m2 = type(m)(**model_kwargs_of({'model_kwargs': kw}))
    assert set(m2.state_dict()) == expect and not torch.equal(m2.planes['xy'], m.planes['xy'])
    m2.load_state_dict(m.state_dict())
    assert all(torch.equal(v, m2.state_dict()[k]) for k, v in m.state_dict().items())
    f = _model(n_comp=4, line_size=11, plane_size=(5, 9))
    assert f.get_kwargs()['line_size'] == 11 and all(tuple(p.shape) == (1, 4, 11, 1) for p in f.lines.values())
    assert all(tuple(p.shape) == (1, 4, 5, 9) for p in f.planes.values())


def test_parameter_shapes_follow_a_non_cubic_world_size():
    m = _model(n_comp=4)
    X, Y, Z = (int(v) for v in m.world_size)
    assert len({X, Y, Z}) == 3
    assert tuple(m.planes['xy'].shape) == (1, 4, Y, Z) and tuple(m.lines['xy'].shape) == (1, 4, X, 1)   # rows y, columns z; line x
    assert tuple(m.planes['yz'].shape) == (1, 4, X, Y) and tuple(m.lines['yz'].shape) == (1, 4, Z, 1)   # rows x, columns y; line z
    assert tuple(m.planes['zx'].shape) == (1, 4, Z, X) and tuple(m.lines['zx'].shape) == (1, 4, Y, 1)   # rows z, columns x; line y
    assert all(p.stride(1) == 1 for p in list(m.planes.values()) + list(m.lines.values()))              # channels-last storage
    cf = _model(n_comp=4, channels_last=False)
    assert all(p.is_contiguous() for p in list(cf.planes.values()) + list(cf.lines.values()))


def test_planes_and_lines_start_non_zero():
    """A product of two zero tensors has a zero gradient for ever."""
    torch.manual_seed(3)
    m = _model(n_comp=4)
    for p in list(m.planes.values()) + list(m.lines.values()):
        assert float(p.detach().abs().min()) > 0 and 0.05 < float(p.detach().std()) < 0.2          # 0.1 * randn
    assert float(m.basis.detach().abs().min()) > 0
    torch.manual_seed(3)
    assert torch.equal(_model(n_comp=4).planes['zx'], m.planes['zx'])              # torch's global generator


def test_sum_and_bad_sizes_raise_value_error():
    with pytest.raises(ValueError, match='tri_aggregation'):
        _model(tri_aggregation='sum')
    _model(tri_aggregation='concat')
    with pytest.raises(ValueError, match='n_comp'):
        _model(n_comp=0)
    with pytest.raises(ValueError, match='line_size'):
        _model(line_size=0)


def test_optimizer_picks_up_planes_lines_and_basis():
    from directvoxgo_amd.train import create_optimizer_or_freeze_model
    from directvoxgo_amd.vm import VM_FINE_TRAIN
    m = _model(n_comp=4)
    opt = create_optimizer_or_freeze_model(m, VM_FINE_TRAIN, global_step=0)
    groups = {id(p): g['lr'] for g in opt.param_groups for p in g['params']}
    assert all(groups[id(p)] == 2e-2 for p in list(m.planes.values()) + list(m.lines.values()))
    assert groups[id(m.basis)] == 1e-3 and groups[id(m.density)] == VM_FINE_TRAIN['lrate_density']
    assert len(groups) == 1 + 3 + 3 + 1 + 6


@pytest.mark.parametrize('kw, match', [
    (dict(implicit_voxel_feat=True), 'implicit_voxel_feat'), (dict(liif=True), 'liif'), (dict(feat_unfold=True), 'feat_unfold'),
    (dict(cell_decode=True), 'cell_decode'), (dict(feat_fourier=True), 'feat_fourier'),
    (dict(posbase_pe=5, cat_posemb=True), 'cat_posemb'), (dict(name='edsr-baseline'), 'encoder'), (dict(rgbnet_dim=0), 'rgbnet_dim')])
def test_the_bases_options_stay_refused(kw, match):
    with pytest.raises(NotImplementedError, match=match):
        _model(**kw)


def test_the_bases_methods_stay_refused(monkeypatch):
    import torch.distributed as dist
    from directvoxgo_amd.export import extract_mesh
    from directvoxgo_amd.pose import CameraRefiner, refine_poses
    from directvoxgo_amd.train import TrainStep
    from directvoxgo_amd.vm import VM_FINE_TRAIN
    m = _model(n_comp=4)
    with pytest.raises(NotImplementedError, match='k0'):
        m.k0_total_variation_add_grad(1.0, True)
    with pytest.raises(NotImplementedError, match='extract_mesh'):
        extract_mesh(m)
    with pytest.raises(NotImplementedError, match='encoder'):
        m.encode_feat(None, None)
    from directvoxgo_amd.scenes import pose_spherical
    poses = pose_spherical(20.0, -30.0, 4.0)[None, :3, :4]
    ref = CameraRefiner(poses, [[8, 8]], [np.array([[8.0, 0, 4], [0, 8.0, 4], [0, 0, 1]], np.float32)])
    with pytest.raises(NotImplementedError, match='VMTriPlaneVoxGO'):
        refine_poses(m, ref, torch.zeros(1, 8, 8, 3), VM_FINE_TRAIN, dict(near=0.1, far=1.0, stepsize=0.5, bg=1), 1, 8, 1e-3)
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_world_size', lambda group=None: 2)
    with pytest.raises(NotImplementedError, match='without k0'):
        TrainStep(m, VM_FINE_TRAIN, dict(near=0.5, far=6.0, bg=1, stepsize=0.5))
