"""CPU: the vector-matrix density's oracle (tests/vm_density_oracle.py) against a float64 torch restatement with autograd,
the forward bound held by the reference alone, the two entry points' typing and argument validation without a device,
and the host side of TensoRFVoxGO."""
import ctypes

import numpy as np
import pytest
import torch

import vm_density_cases as C
import vm_density_oracle as DO
import vm_oracle as VO


def _t64(d, rg=False):
    return {k: torch.from_numpy(v).double().requires_grad_(rg) for k, v in d.items()}


def test_oracle_agrees_with_the_torch_restatement_and_its_autograd():
    """Values and all six gradients to 1e-12 relative (of the largest magnitude of each tensor), on the dyadic case:
    float32 and float64 then see the same cells and weights, and what is left is summation order in float64."""
    mn, mx, xyz, planes, lines, gout = C.dyadic_case(np.random.default_rng(5))
    val, A = DO.forward(planes, lines, xyz, mn, mx)
    rp, rl = _t64(planes, True), _t64(lines, True)
    ref = VO.torch_restatement(rp, rl, torch.from_numpy(xyz).double(), torch.from_numpy(mn).double(),
                               torch.from_numpy(mx).double()).sum(-1)
    ref.backward(torch.from_numpy(gout).double())
    assert val.shape == A.shape == (300,) and (A >= np.abs(val) - 1e-12).all()
    scale = np.abs(ref.detach().numpy()).max()
    assert np.abs(val - ref.detach().numpy()).max() <= 1e-12 * scale
    gp, gl = DO.backward(planes, lines, xyz, mn, mx, gout)
    for k in DO.KEYS:
        for got, t in ((gp[k][0], rp[k].grad[0]), (gl[k][0], rl[k].grad[0, :, :, 0])):
            t = t.numpy()
            assert got.shape == t.shape and np.abs(t).max() > 0
            assert np.abs(got - t).max() <= 1e-12 * np.abs(t).max()


@pytest.mark.parametrize('R', C.RS)
def test_forward_bound_holds_for_the_reference_alone(R):
    """A float32 sum of the float32 products, ascending and pairwise, stays inside (3R + 12) U A on the GPU test's inputs,
    every element: the bound is about float32 arithmetic, not about one implementation's order."""
    planes, lines, per_m = C.case(R)
    for M in C.MS:
        xyz, val, A = per_m[M][:3]
        for order in ('ascending', 'pairwise'):
            got = DO.sum32(planes, lines, xyz, C.MN, C.MX, order).astype(np.float64)
            assert got.shape == val.shape == (M,)
            assert (np.abs(got - val) <= DO.forward_bound(R, A)).all(), (M, order)
    a, b = (DO.sum32(planes, lines, per_m[1000][0], C.MN, C.MX, o) for o in ('ascending', 'pairwise'))
    assert R == 1 or (a != b).any()                                     # the two orders do differ in float32


def test_points_cover_the_edge_cases():
    xyz, val = C.case(4)[2][1000][:2]
    import triplane_oracle as TO
    for key, (H, W) in C.SIZES.items():
        ih, iw, w, ok = TO.corners(key, H, W, xyz, C.MN, C.MX)
        assert ((w == 1).any(0)).sum() >= 8 and (ok[0] & ~ok[2]).any() and (ok[0] & ~ok[1]).any() and (~ok.any(0)).sum() >= 2
    assert (val[[20, 24]] == 0).all() and (val[:20] != 0).any()          # outside on every axis: an exact 0


# ---------------------------------------------------------------------------------------------- build, typing, validation
def test_build_and_typing():
    from directvoxgo_amd import _lib, build
    assert 'vm_density.hip' in build.SOURCES and 'vm_common.h' in build.HEADERS
    build.build(verbose=False)
    with open(_lib.HEADER_PATH) as f:
        decl = _lib.declarations(f.read())
    P, i, q = _lib._Pointer, ctypes.c_int, ctypes.c_int64
    geom = [P, i, i, q, q, q] * 3 + [P, i, q, q] * 3
    assert decl['dvgo_vm_density_fwd'] == (ctypes.c_int, geom + [i, P, P, P, q, P, P])
    assert decl['dvgo_vm_density_bwd'] == (ctypes.c_int, [P] + geom + [P] * 6 + [i, P, P, P, q, i, i, P])
    lib = _lib.lib()
    assert lib.dvgo_vm_density_fwd.argtypes == decl['dvgo_vm_density_fwd'][1]
    assert lib.dvgo_vm_density_bwd.argtypes == decl['dvgo_vm_density_bwd'][1]
    assert _lib.ABI_VERSION == lib.dvgo_abi_version() == 11


@pytest.fixture(scope='module')
def lib():
    from directvoxgo_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


POINTERS = ('xy', 'yz', 'zx', 'xy_line', 'yz_line', 'zx_line', 'xyz', 'mn', 'mx', 'io')
GRADS = ('g_xy', 'g_yz', 'g_zx', 'gl_xy', 'gl_yz', 'gl_zx')
FWD, BWD = 'dvgo_vm_density_fwd', 'dvgo_vm_density_bwd'


def _call(lib, name, M=8, R=4, sizes=((6, 7), (3, 9), (8, 2)), lines=(5, 1, 9), null=(), run=0, mode=0):
    one = ctypes.c_void_p(16)         # any non-null value: rejected before it could be dereferenced, or never reached
    P = lambda k: None if k in null else one         # noqa: E731
    geom = []
    for k, (H, W) in zip(VO.KEYS, sizes):
        geom += [P(k), H, W, 1, W * R, R]
    for k, N in zip(VO.KEYS, lines):
        geom += [P(k + '_line'), N, 1, R]
    tail = [R, P('xyz'), P('mn'), P('mx'), M]
    if name == FWD:
        return lib.dvgo_vm_density_fwd(*geom, *tail, P('io'), None)
    return lib.dvgo_vm_density_bwd(P('io'), *geom, *[P(k) for k in GRADS], *tail, run, mode, None)


@pytest.mark.parametrize('name', [FWD, BWD])
def test_entry_points_validate_before_any_launch(lib, name):
    every = POINTERS + (GRADS if name == BWD else ())
    assert _call(lib, name, M=0) == 0 and _call(lib, name, R=0) == 0                # no-ops
    assert _call(lib, name, M=0, null=every) == 0 and _call(lib, name, R=0, null=every) == 0   # ... that touch no pointer
    assert _call(lib, name, M=-1) == -1 and _call(lib, name, R=-1) == -1
    for k in every:
        assert _call(lib, name, null=(k,)) == -1, k                                  # each pointer is looked at
    assert _call(lib, name, sizes=((6, 7), (0, 9), (8, 2))) == -1                   # a plane axis below 1
    assert _call(lib, name, lines=(5, 0, 9)) == -1 and _call(lib, name, lines=(5, 1, -3)) == -1   # a line length below 1
    assert _call(lib, name, M=0, lines=(5, 0, 9)) == -1                             # sizes are judged before the no-op
    assert _call(lib, name, M=(1 << 31) // 12 + 1) == -2                            # M * 3R >= 2^31
    assert _call(lib, name, M=(1 << 31) // 12 + 1, R=0) == 0


def test_bwd_validates_run_and_mode(lib):
    assert _call(lib, BWD, run=-1) == -1
    assert _call(lib, BWD, mode=-1) == -1 and _call(lib, BWD, mode=3) == -1         # an unknown mode
    assert _call(lib, BWD, M=0, mode=3) == -1 and _call(lib, BWD, M=0, run=-1) == -1
    # mode 2's table is (N_xy + N_yz + N_zx) * R floats; 64 KB is 16384 of them, and one entry more is refused
    assert _call(lib, BWD, M=4, R=4, lines=(2048, 2048, 1), mode=2) == -1
    assert _call(lib, BWD, M=4, R=16, lines=(1024, 1, 1), mode=2) == -1
    assert _call(lib, BWD, M=0, R=4, lines=(2048, 2048, 1), mode=2) == 0            # nothing to do comes first
    from directvoxgo_amd import _lib
    with pytest.raises(RuntimeError, match='invalid argument'):               # the typed call turns the code into an error
        _lib.call(BWD, None, None, 1, 1, 1, 1, 1, None, 1, 1, 1, 1, 1, None, 1, 1, 1, 1, 1, None, 1, 1, 1, None, 1, 1, 1,
                  None, 1, 1, 1, None, None, None, None, None, None, 4, None, None, None, 8, 0, 0, None)
    with pytest.raises(TypeError, match='arguments given'):
        _lib.call(FWD, None, 1, 1)


def test_ops_reject_cpu_tensors_and_bad_arguments():
    from directvoxgo_amd.ops import vm_density
    planes = {k: torch.zeros(1, 4, 5, 6) for k in VO.KEYS}
    lines = {k: torch.zeros(1, 4, 7, 1) for k in VO.KEYS}
    xyz, mn, mx = torch.zeros(7, 3), -torch.ones(3), torch.ones(3)
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        vm_density(planes, lines, xyz, mn, mx)
    with pytest.raises(ValueError, match='three'):
        vm_density(planes, [lines['xy']] * 2, xyz, mn, mx)
    with pytest.raises(RuntimeError, match=r'\[1,R,N,1\]'):
        vm_density(planes, {**lines, 'yz': torch.zeros(1, 4, 7, 2)}, xyz, mn, mx)


# ---------------------------------------------------------------------------------------------- model, host side
BASE = dict(num_voxels=10 * 12 * 14, num_voxels_base=16 ** 3, alpha_init=1e-2, fast_color_thres=1e-4)
BOX = ([-1.0, -1.2, -1.4], [1.0, 1.2, 1.4])
RK = dict(near=0.5, far=6.0, bg=1, stepsize=0.5)


def _model(**kw):
    from directvoxgo_amd.tensorf import TensoRFVoxGO
    return TensoRFVoxGO(*BOX, **{**BASE, **kw})


def test_constructor_kwargs_and_state_dict_round_trip(monkeypatch):
    from directvoxgo_amd.checkpoint import model_kwargs_of
    from directvoxgo_amd.vm import VMTriPlaneVoxGO
    # no dense density tensor during construction either: any [1,1,X,Y,Z] allocation would go through torch.zeros
    zeros, seen = torch.zeros, []
    monkeypatch.setattr(torch, 'zeros', lambda *a, **k: (seen.append(a), zeros(*a, **k))[1])
    m = _model(n_comp=8, density_n_comp=4, rgbnet_dim=6, rgbnet_width=64, density_offset=-2.5)
    monkeypatch.undo()
    ws = [int(v) for v in m.world_size]
    assert not any(list(a[0]) == [1, 1, *ws] for a in seen if a and isinstance(a[0], (list, tuple)))
    assert isinstance(m, VMTriPlaneVoxGO) and m.density is None and not hasattr(m, 'k0')
    sd = set(m.state_dict())
    assert 'density' not in sd
    assert {f'density_planes.{k}' for k in VO.KEYS} | {f'density_lines.{k}' for k in VO.KEYS} <= sd
    assert {'planes.xy', 'lines.zx', 'basis', 'rgbnet.0.weight', 'mask_cache.mask', 'xyz_min'} <= sd
    X, Y, Z = ws
    assert tuple(m.density_planes['xy'].shape) == (1, 4, Y, Z) and tuple(m.density_lines['xy'].shape) == (1, 4, X, 1)
    assert tuple(m.density_planes['zx'].shape) == (1, 4, Z, X) and tuple(m.density_lines['zx'].shape) == (1, 4, Y, 1)
    assert all(p.stride(1) == 1 for p in list(m.density_planes.values()) + list(m.density_lines.values()))
    assert all(0.05 < float(p.detach().std()) < 0.2 for p in m.density_planes.values())          # 0.1 * randn
    kw = m.get_kwargs()
    assert (kw['density_n_comp'], kw['density_plane_size'], kw['density_line_size'], kw['density_offset']) == (4, None, None, -2.5)
    m2 = type(m)(**model_kwargs_of({'model_kwargs': kw}))
    assert m2.density_offset == -2.5 and set(m2.state_dict()) == sd
    m2.load_state_dict(m.state_dict())
    assert all(torch.equal(v, m2.state_dict()[k]) for k, v in m.state_dict().items())
    d = _model()
    assert (d.density_n_comp, d.density_plane_size, d.density_line_size, d.density_offset) == (16, None, None, 0.0)
    f = _model(density_n_comp=2, density_plane_size=(5, 9), density_line_size=11, channels_last=False)
    assert all(tuple(p.shape) == (1, 2, 5, 9) and p.is_contiguous() for p in f.density_planes.values())
    assert all(tuple(p.shape) == (1, 2, 11, 1) for p in f.density_lines.values())
    with pytest.raises(ValueError, match='density_n_comp'):
        _model(density_n_comp=0)
    with pytest.raises(ValueError, match='density_line_size'):
        _model(density_line_size=0)


def test_existing_classes_still_allocate_their_dense_density():
    from directvoxgo_amd.vm import VMTriPlaneVoxGO
    m = VMTriPlaneVoxGO(*BOX, **BASE, n_comp=4)
    assert isinstance(m.density, torch.nn.Parameter) and tuple(m.density.shape[2:]) == tuple(int(v) for v in m.world_size)
    assert 'density' in m.state_dict() and float(m.density.detach().abs().sum()) == 0


def test_optimizer_groups_under_tensorf_fine_train():
    from directvoxgo_amd.tensorf import TENSORF_FINE_TRAIN
    from directvoxgo_amd.train import create_optimizer_or_freeze_model
    from directvoxgo_amd.vm import VM_FINE_TRAIN
    assert TENSORF_FINE_TRAIN == dict(VM_FINE_TRAIN, lrate_density_planes=2e-2, lrate_density_lines=2e-2)
    m = _model(n_comp=4, density_n_comp=4)
    opt = create_optimizer_or_freeze_model(m, TENSORF_FINE_TRAIN, global_step=0)
    groups = {id(p): g['lr'] for g in opt.param_groups for p in g['params']}
    for p in list(m.density_planes.values()) + list(m.density_lines.values()) + list(m.planes.values()) + list(m.lines.values()):
        assert groups[id(p)] == 2e-2
    assert groups[id(m.basis)] == 1e-3 and len(groups) == 3 + 3 + 3 + 3 + 1 + 6       # and no group for `density`


def test_every_refusal_names_the_class(monkeypatch):
    import torch.distributed as dist
    from directvoxgo_amd.export import export_volume, extract_mesh
    from directvoxgo_amd.fit import fit_stage
    from directvoxgo_amd.pose import CameraRefiner, refine_poses
    from directvoxgo_amd.scenes import pose_spherical
    from directvoxgo_amd.tensorf import TENSORF_FINE_TRAIN
    from directvoxgo_amd.train import TrainStep
    m = _model(n_comp=4, density_n_comp=4)
    name = 'TensoRFVoxGO'
    with pytest.raises(NotImplementedError, match=name):
        m.voxel_count_views(None, None, None, 0.1, 1.0, 0.5)
    with pytest.raises(NotImplementedError, match=name + '.*weight_tv_density_planes'):
        m.density_total_variation_add_grad(1.0, True)
    with pytest.raises(NotImplementedError, match=name):
        export_volume(m)
    with pytest.raises(NotImplementedError, match=name):
        extract_mesh(m)
    poses = pose_spherical(20.0, -30.0, 4.0)[None, :3, :4]
    ref = CameraRefiner(poses, [[8, 8]], [np.array([[8.0, 0, 4], [0, 8.0, 4], [0, 0, 1]], np.float32)])
    with pytest.raises(NotImplementedError, match=name):
        refine_poses(m, ref, torch.zeros(1, 8, 8, 3), TENSORF_FINE_TRAIN, dict(near=0.1, far=1.0, stepsize=0.5, bg=1), 1, 8, 1e-3)
    z = torch.zeros(4, 3)
    with pytest.raises(ValueError, match=name):
        fit_stage(m, z, z, z, z, dict(TENSORF_FINE_TRAIN, pervoxel_lr=True), RK, n_iters=1)
    # what the bases refuse stays refused
    with pytest.raises(NotImplementedError, match='k0'):
        m.k0_total_variation_add_grad(1.0, True)
    with pytest.raises(NotImplementedError, match='encoder'):
        m.encode_feat(None, None)
    with pytest.raises(ValueError, match='tri_aggregation'):
        _model(tri_aggregation='sum')
    with pytest.raises(NotImplementedError, match='liif'):
        _model(liif=True)
    assert not m.can_keep_count_on_device() and not TrainStep(m, dict(TENSORF_FINE_TRAIN), RK).can_capture()
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_world_size', lambda group=None: 2)
    with pytest.raises(NotImplementedError, match=name):
        TrainStep(m, TENSORF_FINE_TRAIN, RK)


@pytest.mark.parametrize('key', ['weight_tv_density_planes', 'weight_tv_density_lines', 'weight_l1_density_planes',
                                 'weight_l1_density_lines'])
def test_density_regulariser_keys_need_density_planes(key):
    from directvoxgo_amd.tensorf import TENSORF_FINE_TRAIN
    from directvoxgo_amd.train import DENSITY_REG_KEYS, TrainStep
    from directvoxgo_amd.vm import VM_FINE_TRAIN, VMTriPlaneVoxGO
    assert key in DENSITY_REG_KEYS
    vm = VMTriPlaneVoxGO(*BOX, **BASE, n_comp=4)
    with pytest.raises(ValueError, match=key + '.*VMTriPlaneVoxGO'):
        TrainStep(vm, dict(VM_FINE_TRAIN, **{key: 1e-3}), RK)
    assert not TrainStep(vm, dict(VM_FINE_TRAIN, **{key: 0.0}), RK).density_reg_on          # absent or 0: nothing
    step = TrainStep(_model(n_comp=4, density_n_comp=4), dict(TENSORF_FINE_TRAIN, **{key: 1e-3}), RK)
    assert step.density_reg_on and step._tv_weighted() and not step.plane_reg_on
