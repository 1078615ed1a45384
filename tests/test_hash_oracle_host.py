"""CPU: the hash-grid sampler's level table, its oracle (tests/hash_oracle.py) against a brute-force float64 restatement
and against a finite difference of itself, the build and typing of the two entry points, their argument validation without
a device, and the host side of HashVoxGO."""
import ctypes

import numpy as np
import pytest
import torch

import hash_oracle as HO

MN, MX = np.array([-1.0, -0.8, -0.6], np.float32), np.array([0.9, 1.1, 0.7], np.float32)
# dense, dense, hashed into 16 rows (collisions, same-cell ones included), hashed into 2^10
RES = np.array([[2, 2, 2], [2, 3, 7], [9, 9, 9], [33, 17, 40]], np.int32)
OFFSETS = np.cumsum([0, 8, 42, 16, 1024]).astype(np.int64)


# ---------------------------------------------------------------------------------------------- the level table
def _levels(*a, **kw):
    from directvoxgo_amd.hashgrid import hash_levels
    res, off = hash_levels(*a, **kw)
    assert res.dtype == torch.int32 and off.dtype == torch.int64
    return res.numpy(), off.numpy()


def test_hash_levels_of_a_cube():
    res, off = _levels([-1, -1, -1], [1, 1, 1], n_levels=16, base_res=16, max_res=512, log2_hashmap_size=19)
    assert res.shape == (16, 3) and off.shape == (17,) and off[0] == 0
    assert (res[:, 0] == res[:, 1]).all() and (res[:, 0] == res[:, 2]).all()
    assert res[0, 0] == 16 and res[-1, 0] == 512 and (np.diff(res[:, 0]) > 0).all()          # monotone, both ends exact
    s = 16.0 * 32.0 ** (np.arange(16) / 15.0)
    assert (res[:, 0] == np.floor(s + 0.5).astype(np.int64)).all()
    size = np.diff(off)
    nodes = res.astype(np.int64).prod(1)
    dense = nodes <= 2 ** 19
    assert (size[dense] == nodes[dense]).all() and (size[~dense] == 2 ** 19).all()
    assert res[6, 0] == 64 and res[7, 0] == 81                    # 64^3 = 2^18 fits, 81^3 = 531441 > 2^19 does not:
    assert dense[:7].all() and not dense[7:].any()                # the split, and no way back
    for l in range(16):
        assert HO.level_size(res, off, l) == (int(size[l]), not dense[l])
    assert off[-1] * 2 * 4 < 2 ** 26                              # 16 x 2^19 x 2 floats is the bound: 64 MB


def test_hash_levels_single_level_and_anisotropic_boxes():
    res, off = _levels([0, 0, 0], [1, 1, 1], n_levels=1, base_res=5, max_res=99, log2_hashmap_size=4)
    assert res.tolist() == [[5, 5, 5]] and off.tolist() == [0, 16]                     # s_0 = base_res; 125 nodes hashed into 16
    res, off = _levels([0, 0, 0], [4, 2, 0.1], n_levels=3, base_res=4, max_res=16, log2_hashmap_size=8)
    assert res.tolist() == [[4, 2, 2], [8, 4, 2], [16, 8, 2]]                          # the longest axis gets s_l; never below 2
    assert off.tolist() == [0, 16, 80, 336]
    res2, off2 = _levels(torch.tensor([0., 0, 0]), torch.tensor([4., 2, 0.1]), n_levels=3, base_res=4, max_res=16,
                         log2_hashmap_size=8)
    assert (res2 == res).all() and (off2 == off).all()
    # rounding to nearest, on the float32 box taken to float64
    res, _ = _levels(MN, MX, n_levels=2, base_res=10, max_res=21, log2_hashmap_size=30)
    ext = MX.astype(np.float64) - MN.astype(np.float64)
    for l, s in enumerate((10.0, 21.0)):
        assert res[l].tolist() == np.maximum(2, np.floor(s * ext / ext.max() + 0.5)).astype(int).tolist()
    for bad in (dict(n_levels=0), dict(n_levels=33), dict(base_res=8, max_res=4), dict(base_res=1), dict(log2_hashmap_size=32)):
        with pytest.raises(ValueError):
            _levels([0, 0, 0], [1, 1, 1], **{**dict(n_levels=2, base_res=4, max_res=8, log2_hashmap_size=4), **bad})


# ---------------------------------------------------------------------------------------------- the oracle
def _points(rng, n):
    return (MN + (MX - MN) * (rng.random((n, 3)) * 1.2 - 0.1)).astype(np.float32)       # up to 10 % outside


def test_oracle_agrees_with_the_brute_force_restatement():
    """Every level expanded to a dense array by looking each node up, then float64 trilinear interpolation.  The two differ
    by the float32 coordinate only: five float32 operations put g within 5 u R of its real value, the interpolant's slope
    along an axis is at most the largest difference of two nodes, 2 max|v|, and there are three axes."""
    rng = np.random.default_rng(5)
    F = 2
    table = rng.standard_normal((int(OFFSETS[-1]), F)).astype(np.float32)
    xyz = np.concatenate([_points(rng, 600), MN[None], MX[None]])
    val, A = HO.forward(table, xyz, MN, MX, RES, OFFSETS)
    assert val.shape == A.shape == (602, 4 * F) and (A >= np.abs(val) - 1e-12).all()
    ref = HO.brute_force(table, xyz, MN, MX, RES, OFFSETS)
    tol = 3 * (5 * HO.U * RES.max()) * 2 * np.abs(table).max()
    print('worst |oracle - brute force|:', float(np.abs(val - ref).max()), 'allowed', float(tol))
    assert np.abs(val - ref).max() <= tol
    # on the box's corners the value is the corner node's row, exactly
    for l in range(4):
        lo = HO.dense_expansion(table, RES, OFFSETS, l)[0, 0, 0]
        hi = HO.dense_expansion(table, RES, OFFSETS, l)[-1, -1, -1]
        assert (val[600, l * F:(l + 1) * F] == lo).all() and (val[601, l * F:(l + 1) * F] == hi).all()
    # the hashed levels collide, inside one cell too; the dense ones never do
    assert HO.same_cell_collisions(RES, OFFSETS, 2, xyz, MN, MX) > 0
    assert HO.same_cell_collisions(RES, OFFSETS, 0, xyz, MN, MX) == HO.same_cell_collisions(RES, OFFSETS, 1, xyz, MN, MX) == 0
    ix, iy, iz = np.meshgrid(np.arange(9), np.arange(9), np.arange(9), indexing='ij')
    assert np.unique(HO.node_rows(RES, OFFSETS, 2, ix, iy, iz)).size == 16 < 729


def test_hash_rows_wrap_at_32_bits():
    """The products wrap at 2^32 before the xor; a lattice large enough to tell that from exact products."""
    res, off = np.array([[4, 70000, 70000]], np.int32), np.array([0, 1 << 20], np.int64)
    iy, iz = np.array([3, 65535, 69999]), np.array([69999, 7, 65537])
    got = HO.node_rows(res, off, 0, np.array([1, 2, 3]), iy, iz)
    for k in range(3):
        h = (int([1, 2, 3][k]) * 1) % 2 ** 32 ^ (int(iy[k]) * 2654435761) % 2 ** 32 ^ (int(iz[k]) * 805459861) % 2 ** 32
        assert got[k] == h & ((1 << 20) - 1)
        assert (int(iy[k]) * 2654435761) >= 2 ** 32 or k == 0
    with pytest.raises(ValueError):
        HO.level_size(np.array([[3, 3, 3]]), np.array([0, 12]), 0)                      # neither 27 nor a power of two
    with pytest.raises(ValueError):
        HO.level_size(np.array([[3, 3, 3]]), np.array([0, 32]), 0)                      # a power of two, but above 27


def test_oracle_backward_is_the_derivative_of_its_forward():
    """In float64.  The forward is linear in the table, so a central difference is exact up to rounding."""
    rng = np.random.default_rng(6)
    F = 4
    T = int(OFFSETS[-1])
    table = rng.standard_normal((T, F))
    xyz = _points(rng, 300)
    g = rng.standard_normal((300, 4 * F))
    grad, A, n = HO.backward((T, F), xyz, MN, MX, RES, OFFSETS, g)
    assert grad.shape == A.shape == (T, F) and n.shape == (T,) and n.sum() == 300 * 4 * 8
    # (a clamped sample reaches its upper nodes with a weight of exactly 0: a row may be counted and still have A == 0)
    assert (A[n == 0] == 0).all() and (grad[n == 0] == 0).all() and (n == 0).any() and (A[n > 0] > 0).any()
    touched = np.flatnonzero(n)
    for k in np.concatenate([rng.choice(touched, 40), rng.choice(np.flatnonzero(n == 0), 3), np.arange(8)]):
        c = int(rng.integers(F))
        d = np.zeros((T, F)); d[k, c] = 0.5
        fd = ((HO.forward(table + d, xyz, MN, MX, RES, OFFSETS)[0] - HO.forward(table - d, xyz, MN, MX, RES, OFFSETS)[0]) * g).sum()
        assert abs(fd - grad[k, c]) <= 1e-10 * max(1.0, A[k, c]), (k, c, fd, grad[k, c])
    # and the adjoint identity over the whole table
    lhs, rhs = (grad * table).sum(), (HO.forward(table, xyz, MN, MX, RES, OFFSETS)[0] * g).sum()
    assert abs(lhs - rhs) <= 1e-9 * np.abs(grad * table).sum()


# ---------------------------------------------------------------------------------------------- build, typing, validation
def test_build_and_typing():
    from directvoxgo_amd import _lib, build
    assert 'hashgrid.hip' in build.SOURCES
    build.build(verbose=False)
    with open(_lib.HEADER_PATH) as f:
        decl = _lib.declarations(f.read())
    P, i, q = _lib._Pointer, ctypes.c_int, ctypes.c_int64
    assert decl['dvgo_hash_fwd'] == (ctypes.c_int, [P, i, i, P, P, P, P, P, q, P, P])
    assert decl['dvgo_hash_bwd'] == (ctypes.c_int, [P, P, i, i, P, P, P, P, P, q, i, i, P])
    lib = _lib.lib()
    assert lib.dvgo_hash_fwd.argtypes == decl['dvgo_hash_fwd'][1] and lib.dvgo_hash_bwd.argtypes == decl['dvgo_hash_bwd'][1]
    assert _lib.ABI_VERSION == lib.dvgo_abi_version()


@pytest.fixture(scope='module')
def lib():
    from directvoxgo_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


POINTERS = ('table', 'xyz', 'mn', 'mx', 'io')


def _call(lib, name, M=8, F=2, res=RES, offsets=OFFSETS, null=(), run=0, mode=0, addr=64):
    one = ctypes.c_void_p(addr)       # any non-null value: rejected before it could be dereferenced, or never reached
    P = lambda k: None if k in null else one         # noqa: E731
    L = len(res) if res is not None else 1
    c_res = None if res is None else (ctypes.c_int32 * (3 * L))(*[int(v) for v in np.asarray(res).reshape(-1)])
    c_off = None if offsets is None else (ctypes.c_int64 * len(offsets))(*[int(v) for v in offsets])
    if name == 'dvgo_hash_fwd':
        return lib.dvgo_hash_fwd(P('table'), F, L, c_res, c_off, P('xyz'), P('mn'), P('mx'), M, P('io'), None)
    return lib.dvgo_hash_bwd(P('io'), P('table'), F, L, c_res, c_off, P('xyz'), P('mn'), P('mx'), M, run, mode, None)


@pytest.mark.parametrize('name', ['dvgo_hash_fwd', 'dvgo_hash_bwd'])
def test_entry_points_validate_before_any_launch(lib, name):
    assert _call(lib, name, M=0) == 0 and _call(lib, name, M=0, null=POINTERS) == 0     # a no-op that touches no pointer
    assert _call(lib, name, M=-1) == -1
    for k in POINTERS:
        assert _call(lib, name, null=(k,)) == -1, k                                      # each pointer is looked at
    for F in (0, 3, 5, 6, 7, 16, -2):
        assert _call(lib, name, F=F) == -1 and _call(lib, name, M=0, F=F) == -1          # judged before the no-op
    assert _call(lib, name, res=None) == -1 and _call(lib, name, offsets=None) == -1
    assert _call(lib, name, M=0, res=[[2, 1, 2]], offsets=[0, 4]) == -1                  # a node count below 2
    assert _call(lib, name, M=0, res=[[3, 3, 3]], offsets=[0, 12]) == -1                 # neither 27 nor a power of two
    assert _call(lib, name, M=0, res=[[3, 3, 3]], offsets=[0, 32]) == -1                 # a power of two above the node count
    assert _call(lib, name, M=0, res=[[3, 3, 3]], offsets=[0, 0]) == -1 and _call(lib, name, M=0, res=[[3, 3, 3]], offsets=[5, 2]) == -1
    assert _call(lib, name, M=0, res=[[3, 3, 3]], offsets=[-1, 26]) == -1
    for size in (27, 16, 1):
        assert _call(lib, name, M=0, res=[[3, 3, 3]], offsets=[7, 7 + size]) == 0
    many = [[2, 2, 2]] * 33
    assert _call(lib, name, M=0, res=many, offsets=list(range(0, 8 * 34, 8))) == -1       # more than 32 levels
    assert _call(lib, name, M=0, res=many[:32], offsets=list(range(0, 8 * 33, 8))) == 0
    assert _call(lib, name, M=(1 << 31) // 8 + 1) == -2                                  # M * L * F >= 2^31
    assert _call(lib, name, M=0, res=[[65536, 32768, 2]], offsets=[0, 16]) == -2         # Rx Ry >= 2^31


def test_alignment_is_checked_before_any_launch(lib):
    """A misaligned table or output is refused; an aligned one would launch, which a machine without a device answers with
    a HIP error (positive) or, with one, would dereference the made-up address: only the refusals are called."""
    for name in ('dvgo_hash_fwd', 'dvgo_hash_bwd'):
        for F, addr in ((2, 4), (4, 8), (8, 8), (8, 4), (1, 2)):
            assert _call(lib, name, F=F, addr=addr) == -1, (name, F, addr)


def test_bwd_validates_run_and_mode(lib):
    name = 'dvgo_hash_bwd'
    assert _call(lib, name, run=-1) == -1 and _call(lib, name, M=0, run=-1) == -1
    assert _call(lib, name, mode=-1) == -1 and _call(lib, name, mode=4) == -1 and _call(lib, name, M=0, mode=4) == -1
    assert _call(lib, name, M=(1 << 31) // 32, F=1, mode=2) == -2                        # mode 2: 8 M L >= 2^31
    assert all(_call(lib, name, M=0, mode=mode) == 0 for mode in (0, 1, 2, 3))
    from directvoxgo_amd import _lib
    with pytest.raises(RuntimeError, match='invalid argument'):               # the typed call turns the code into an error
        _lib.call('dvgo_hash_bwd', None, None, 3, 1, None, None, None, None, None, 8, 0, 0, None)


def test_ops_reject_cpu_tensors_and_bad_tables():
    from directvoxgo_amd.ops import HashLevels, hash_sample
    xyz, mn, mx = torch.zeros(7, 3), -torch.ones(3), torch.ones(3)
    table = torch.zeros(int(OFFSETS[-1]), 2)
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        hash_sample(table, xyz, mn, mx, torch.from_numpy(RES), torch.from_numpy(OFFSETS))
    with pytest.raises(ValueError, match='F in'):
        hash_sample(torch.zeros(int(OFFSETS[-1]), 3), xyz, mn, mx, RES, OFFSETS)
    with pytest.raises(ValueError, match='rows'):
        hash_sample(table[:-1], xyz, mn, mx, RES, OFFSETS)
    with pytest.raises(ValueError, match='power of two'):
        hash_sample(table, xyz, mn, mx, [[3, 3, 3]], [0, 12])
    with pytest.raises(ValueError, match='power of two'):
        hash_sample(table, xyz, mn, mx, [[3, 3, 3]], [0, 32])
    with pytest.raises(ValueError, match='at least 2'):
        hash_sample(table, xyz, mn, mx, [[3, 1, 3]], [0, 8])
    with pytest.raises(ValueError, match='L'):
        hash_sample(table, xyz, mn, mx, [[3, 3, 3]], [0, 8, 16])
    lv = HashLevels(RES, OFFSETS)
    assert lv.L == 4 and lv.rows == int(OFFSETS[-1]) and lv.hashed == [False, False, True, True]
    assert list(lv.c_res) == RES.reshape(-1).tolist() and list(lv.c_offsets) == OFFSETS.tolist()


# ---------------------------------------------------------------------------------------------- model, host side
BASE = dict(num_voxels=10 * 12 * 14, num_voxels_base=16 ** 3, alpha_init=1e-2, fast_color_thres=1e-4)
BOX = ([-1.0, -1.2, -1.4], [1.0, 1.2, 1.4])
SMALL = dict(n_levels=4, n_feat=2, log2_hashmap_size=10, base_res=4, max_res=32)


def _model(**kw):
    from directvoxgo_amd.hashgrid import HashVoxGO
    return HashVoxGO(*BOX, **{**BASE, **SMALL, **kw})


def test_constructor_kwargs_and_state_dict_round_trip():
    from directvoxgo_amd.checkpoint import model_kwargs_of
    from directvoxgo_amd.hashgrid import HashVoxGO, hash_levels
    from directvoxgo_amd.voxel_model import VoxelModel
    torch.manual_seed(2)
    m = _model(rgbnet_width=64)
    assert isinstance(m, VoxelModel) and not hasattr(m, 'k0') and not hasattr(m, 'planes')
    expect = {'xyz_min', 'xyz_max', 'density', 'viewfreq', 'hash_table', 'rgbnet.0.weight', 'rgbnet.0.bias', 'rgbnet.2.0.weight',
              'rgbnet.2.0.bias', 'rgbnet.3.weight', 'rgbnet.3.bias', 'mask_cache.mask', 'mask_cache.xyz2ijk_scale',
              'mask_cache.xyz2ijk_shift'}
    assert set(m.state_dict()) == expect
    res, off = hash_levels(*BOX, **{k: v for k, v in SMALL.items() if k != 'n_feat'})
    assert m.levels.res == res.tolist() and m.levels.offsets == off.tolist()
    assert tuple(m.hash_table.shape) == (int(off[-1]), 2) and m.hash_table.is_contiguous()
    t = m.hash_table.detach()
    assert float(t.abs().max()) <= 1e-4 and float(t.std()) > 4e-5 and float(t.mean().abs()) < 1e-5      # U(-1e-4, 1e-4)
    torch.manual_seed(2)
    assert torch.equal(_model(rgbnet_width=64).hash_table, m.hash_table)            # torch's global generator
    assert m.feat_dim == 8 and m.rgbnet[0].in_features == 8 - 3 + 27
    assert _model(rgbnet_direct=True).rgbnet[0].in_features == 8 + 27
    kw = m.get_kwargs()
    assert {k: kw[k] for k in SMALL} == SMALL and 'rgbnet_dim' not in kw and 'tri_aggregation' not in kw
    m2 = HashVoxGO(**model_kwargs_of({'model_kwargs': kw}))
    assert set(m2.state_dict()) == expect and not torch.equal(m2.hash_table, m.hash_table)
    m2.load_state_dict(m.state_dict())
    assert all(torch.equal(v, m2.state_dict()[k]) for k, v in m.state_dict().items())
    assert m2.levels.res == m.levels.res and m2.levels.offsets == m.levels.offsets


def test_defaults_are_the_papers():
    import inspect
    from directvoxgo_amd.hashgrid import HASH_FINE_TRAIN, HashVoxGO
    from directvoxgo_amd.train import FINE_TRAIN
    sig = inspect.signature(HashVoxGO.__init__).parameters
    assert {k: sig[k].default for k in ('n_levels', 'n_feat', 'log2_hashmap_size', 'base_res', 'max_res')} == \
        dict(n_levels=16, n_feat=2, log2_hashmap_size=19, base_res=16, max_res=512)
    assert HASH_FINE_TRAIN == dict(FINE_TRAIN, lrate_hash_table=1e-2, skip_zero_grad_fields=['density', 'hash_table'])


def test_bad_options_raise_value_error():
    for bad, match in ((dict(n_feat=3), 'n_feat'), (dict(n_feat=16), 'n_feat'), (dict(n_levels=0), 'n_levels'),
                       (dict(base_res=16, max_res=8), 'max_res'), (dict(n_levels=1, n_feat=2), 'diffuse')):
        with pytest.raises(ValueError, match=match):
            _model(**bad)
    assert _model(n_levels=1, n_feat=2, rgbnet_direct=True).feat_dim == 2


def test_optimizer_picks_up_the_table():
    from directvoxgo_amd.hashgrid import HASH_FINE_TRAIN
    from directvoxgo_amd.train import create_optimizer_or_freeze_model
    m = _model()
    opt = create_optimizer_or_freeze_model(m, HASH_FINE_TRAIN, global_step=0)
    groups = {id(p): g for g in opt.param_groups for p in g['params']}
    assert groups[id(m.hash_table)]['lr'] == 1e-2 and groups[id(m.hash_table)]['skip_zero_grad'] is True
    assert groups[id(m.density)]['lr'] == HASH_FINE_TRAIN['lrate_density'] and groups[id(m.density)]['skip_zero_grad'] is True
    assert len(groups) == 1 + 1 + 6 and not groups[id(m.rgbnet[0].weight)]['skip_zero_grad']


def test_what_is_left_out_raises_and_names_the_class(monkeypatch):
    import torch.distributed as dist
    from directvoxgo_amd.export import extract_mesh
    from directvoxgo_amd.hashgrid import HASH_FINE_TRAIN
    from directvoxgo_amd.pose import CameraRefiner, refine_poses
    from directvoxgo_amd.scenes import pose_spherical
    from directvoxgo_amd.train import TrainStep
    m = _model()
    with pytest.raises(NotImplementedError, match='HashVoxGO'):
        m.k0_total_variation_add_grad(1.0, True)
    with pytest.raises(NotImplementedError, match='extract_mesh.*HashVoxGO'):
        extract_mesh(m)
    with pytest.raises(NotImplementedError, match='posbase_pe.*HashVoxGO'):
        _model(posbase_pe=5)
    poses = pose_spherical(20.0, -30.0, 4.0)[None, :3, :4]
    ref = CameraRefiner(poses, [[8, 8]], [np.array([[8.0, 0, 4], [0, 8.0, 4], [0, 0, 1]], np.float32)])
    with pytest.raises(NotImplementedError, match='refine_poses: HashVoxGO'):
        refine_poses(m, ref, torch.zeros(1, 8, 8, 3), HASH_FINE_TRAIN, dict(near=0.1, far=1.0, stepsize=0.5, bg=1), 1, 8, 1e-3)
    with pytest.raises(ValueError, match='HashVoxGO has no planes'):
        m.plane_regularizers_add_grad(True, weight_tv_planes=1.0)
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_world_size', lambda group=None: 2)
    with pytest.raises(NotImplementedError, match='data-parallel training of HashVoxGO'):
        TrainStep(m, HASH_FINE_TRAIN, dict(near=0.5, far=6.0, bg=1, stepsize=0.5))
