"""CPU: the hash sampler's position gradient (csrc/hash_xyz.hip) without a device.

  * tests/hash_raygrad_oracle.py equals float64 torch.autograd of a torch restatement of the sampler at points whose float32
    and float64 cells agree (box [-1, 1]^3, node counts 2^k + 1, coordinates on multiples of 2^-10: every float32 coordinate
    operation is exact), lattice planes included; outside the box it equals a central difference of hash_oracle.forward:
    zero along the clamped axes, the face's derivative along the others;
  * the kernel's arithmetic restated in float32 numpy stays inside the bound the GPU test applies to the kernel, and planted
    mistakes leave it;
  * the boundary: the declaration parses, _lib types the entry, the library exports it, the staged error codes and the
    M == 0 no-op answer with null pointers;
  * host logic: `raygrad` is no get_kwargs key and survives load_model, the default model's refusal names the class and carries
    the hint, refine_poses(fused=True) is a ValueError.
"""
import ctypes

import numpy as np
import pytest
import torch

import hash_oracle as HO
import hash_raygrad_oracle as HR

f32 = np.float32
MN1, MX1 = f32([-1, -1, -1]), f32([1, 1, 1])
RES1 = np.array([[3, 5, 9], [17, 9, 33], [5, 5, 5]], np.int32)
OFF1 = np.array([0, 135, 135 + 256, 135 + 256 + 8], np.int64)


def _torch_restatement(table, xyz, mn, mx, res, off):
    """tests/test_gpu_hash.py's: every level expanded to a dense [1,F,X,Y,Z] array by looking each node up, then
    F.grid_sample (trilinear, align_corners=True), in float64; differentiable in `xyz`.  For points with g < R - 1, where the
    padding is not reached (grid_sample's backward takes the floor's cell too, so lattice planes agree)."""
    import torch.nn.functional as Fn
    ind = ((xyz - mn) / (mx - mn)).flip((-1,)) * 2 - 1
    out = []
    for l in range(len(res)):
        X, Y, Z = (int(v) for v in res[l])
        ix, iy, iz = np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing='ij')
        rows = torch.from_numpy(int(off[l]) + HO.node_rows(res, off, l, ix, iy, iz))
        dense = table[rows].permute(3, 0, 1, 2)[None]
        out.append(Fn.grid_sample(dense, ind.reshape(1, 1, 1, -1, 3), mode='bilinear', align_corners=True)[0, :, 0, 0].T)
    return torch.cat(out, -1)


def test_oracle_equals_float64_autograd_where_the_cells_agree():
    rng = np.random.default_rng(3)
    Fc, M = 2, 400
    table = (0.5 * rng.standard_normal((int(OFF1[-1]), Fc))).astype(f32)
    xyz = (rng.integers(-1024, 1024, (M, 3)) / 1024.0).astype(f32)               # g < R - 1: the padding is not reached
    xyz[:40] = (rng.integers(-4, 4, (40, 3)) / 4.0).astype(f32)                   # on lattice planes of every level
    gout = rng.standard_normal((M, len(RES1) * Fc)).astype(f32)
    x64 = torch.from_numpy(xyz).double().requires_grad_(True)
    ref = _torch_restatement(torch.from_numpy(table).double(), x64, torch.from_numpy(MN1).double(), torch.from_numpy(MX1).double(),
                             RES1, OFF1)
    ref.backward(torch.from_numpy(gout).double())
    S = HR.sums(table, gout, xyz, MN1, MX1, RES1, OFF1)
    assert HO.same_cell_collisions(RES1, OFF1, 2, xyz, MN1, MX1) > 0             # two corners on one row are two terms
    err = np.abs(S.ref - x64.grad.numpy())
    print('worst |oracle - autograd|:', float(err.max()), 'largest mag', float(S.mag.max()))
    assert (err <= 1e-12 * (1.0 + S.mag)).all()
    assert (S.mag >= np.abs(S.ref) - 1e-12).all() and (S.mag > 0).all()


def test_oracle_outside_the_box_equals_a_central_difference_of_the_forward():
    """hash_oracle.forward clamps, so beyond a face it is constant along that axis and keeps the face's values along the
    others.  Dyadic coordinates and a step of 2^-8 that stays inside one cell (or inside the clamped region): the float32
    coordinates are exact and the piecewise-trilinear function is linear along the step, so the difference is exact."""
    rng = np.random.default_rng(4)
    Fc, M, h = 2, 240, 2.0 ** -8
    table = (0.5 * rng.standard_normal((int(OFF1[-1]), Fc))).astype(f32)
    gout = rng.standard_normal((M, len(RES1) * Fc)).astype(f32)
    # inside coordinates on odd multiples of 2^-7 (never on a lattice plane of 3..33 nodes over [-1, 1], never within h of one)
    xyz = ((2 * rng.integers(-64, 64, (M, 3)) + 1) / 128.0).astype(np.float64)
    out = np.where(rng.integers(0, 2, (M, 3)) == 1, 1.0 + rng.integers(2, 64, (M, 3)) / 64.0, -1.0 - rng.integers(2, 64, (M, 3)) / 64.0)
    n_out = np.arange(M) % 4                                                      # 0, 1, 2 or 3 axes outside
    clamp = np.zeros((M, 3), bool)
    for m in range(M):
        clamp[m, rng.permutation(3)[:n_out[m]]] = True
    xyz = np.where(clamp, out, xyz).astype(f32)
    S = HR.sums(table, gout, xyz, MN1, MX1, RES1, OFF1)
    assert (S.ref[clamp] == 0).all() and (S.mag[clamp] == 0).all() and (S.mag[~clamp] > 0).all()
    g64 = gout.astype(np.float64)
    for a in range(3):
        d = np.zeros(3, f32); d[a] = h
        fd = ((HO.forward(table, xyz + d, MN1, MX1, RES1, OFF1)[0] - HO.forward(table, xyz - d, MN1, MX1, RES1, OFF1)[0]) * g64).sum(1) / (2 * h)
        assert (np.abs(fd - S.ref[:, a]) <= 1e-9 * (1.0 + S.mag[:, a])).all(), a
        assert (fd[clamp[:, a]] == 0).all()
    assert all((clamp.sum(1) == k).any() for k in (0, 1, 2, 3))


@pytest.mark.parametrize('name', ['dense_and_hashed', 'L5_mixed', 'one_2x2x2'])
def test_float32_restatement_is_inside_the_bound_and_planted_mistakes_are_not(name):
    res, off = HR.LEVEL_TABLES[name]
    Fc, M = 2, 257
    table = HR.table_values(int(off[-1]), Fc, 7)
    xyz = HR.points(M, 8)
    gout = HR.grad_values(M, len(res) * Fc, 9)
    S = HR.sums(table, gout, xyz, HR.MN, HR.MX, res, off)
    fam = np.arange(M) % HR.N_FAMILIES
    assert (S.mag[fam == 8] == 0).all() and (S.mag[fam == 7] == 0).all() and (S.mag[fam <= 4] > 0).all()
    worst = HR.check(S, HR.evaluate32(table, gout, xyz, HR.MN, HR.MX, res, off))
    print(name, 'float32 restatement: worst err / bound', worst)
    for planted in (dict(drop_corner=5), dict(flip_axis=1), dict(no_scale=True), dict(no_clamp=True)):
        with pytest.raises(AssertionError):
            HR.check(S, HR.evaluate32(table, gout, xyz, HR.MN, HR.MX, res, off, **planted))
    with pytest.raises(AssertionError, match='non-finite'):
        HR.check(S, np.full((M, 3), np.nan, f32))


def test_point_families_are_present():
    res, off = HR.LEVEL_TABLES['dense_and_hashed']
    xyz = HR.points(257, 8)
    I = HR.inputs32(xyz, HR.MN, HR.MX, res, 0)
    R1 = np.asarray(res[0]) - 1
    on_plane = (I.w[:, :, 1] == 0) & (I.f > 0) & I.inside                        # g an interior node: the upper cell, weight 1 on its floor
    assert on_plane.any(0).all() and on_plane.all(1).any()
    lo = I.inside & (I.f == 0) & (I.w[:, :, 1] == 0)
    hi = I.inside & (I.f == R1 - 1) & (I.w[:, :, 1] == 1)                        # g == R - 1: the last cell, weight 1 on its upper node
    assert lo.any(0).all() and hi.any(0).all()
    finite = ~np.isnan(xyz).any(1)
    n_out = (~I.inside[finite]).sum(1)
    assert all((n_out == k).any() for k in (0, 1, 2, 3)) and (~finite).sum() >= 1


# ---------------------------------------------------------------------------------------------- boundary
@pytest.fixture(scope='module')
def lib():
    from directvoxgo_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def test_header_declares_the_entry_and_lib_types_it(lib):
    from directvoxgo_amd import _lib, build
    assert 'hash_xyz.hip' in build.SOURCES and 'hashgrid.hip' in build.SOURCES and 'hash_common.h' in build.HEADERS
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    decl = _lib.declarations(text)
    P, i, q = _lib._Pointer, ctypes.c_int, ctypes.c_int64
    assert decl['dvgo_hash_bwd_xyz'] == (ctypes.c_int, [P, i, i, P, P, P, P, P, P, q, P, P])
    assert lib.dvgo_hash_bwd_xyz.argtypes == decl['dvgo_hash_bwd_xyz'][1] and lib.dvgo_hash_bwd_xyz.restype is ctypes.c_int
    assert ctypes.CDLL(_lib.SO_PATH).dvgo_hash_bwd_xyz                              # exported
    assert _lib.ABI_VERSION == lib.dvgo_abi_version() == 11                         # no bump
    assert 'No gradient for xyz' in text and 'dvgo_hash_bwd_xyz entries were added' in text


POINTERS = ('table', 'gout', 'xyz', 'mn', 'mx', 'gxyz')
RES = np.array([[2, 2, 2], [2, 3, 7], [9, 9, 9], [33, 17, 40]], np.int32)
OFFSETS = np.cumsum([0, 8, 42, 16, 1024]).astype(np.int64)


def _call(lib, M=8, F=2, res=RES, offsets=OFFSETS, null=(), addr=64):
    one = ctypes.c_void_p(addr)       # any non-null value: rejected before it could be dereferenced, or never reached
    P = lambda k: None if k in null else one         # noqa: E731
    L = len(res) if res is not None else 1
    c_res = None if res is None else (ctypes.c_int32 * (3 * L))(*[int(v) for v in np.asarray(res).reshape(-1)])
    c_off = None if offsets is None else (ctypes.c_int64 * len(offsets))(*[int(v) for v in offsets])
    return lib.dvgo_hash_bwd_xyz(P('table'), F, L, c_res, c_off, P('gout'), P('xyz'), P('mn'), P('mx'), M, P('gxyz'), None)


def test_entry_validates_before_any_launch(lib):
    """The conditions and codes of tests/test_hash_oracle_host.py for dvgo_hash_fwd, in the same order."""
    assert _call(lib, M=0) == 0 and _call(lib, M=0, null=POINTERS) == 0                  # a no-op that touches no pointer
    assert _call(lib, M=-1) == -1
    for k in POINTERS:
        assert _call(lib, null=(k,)) == -1, k                                            # each pointer is looked at
    for F in (0, 3, 5, 6, 7, 16, -2):
        assert _call(lib, F=F) == -1 and _call(lib, M=0, F=F) == -1                      # judged before the no-op
    assert _call(lib, res=None) == -1 and _call(lib, offsets=None) == -1
    assert _call(lib, M=0, res=[[2, 1, 2]], offsets=[0, 4]) == -1                        # a node count below 2
    assert _call(lib, M=0, res=[[3, 3, 3]], offsets=[0, 12]) == -1                       # neither 27 nor a power of two
    assert _call(lib, M=0, res=[[3, 3, 3]], offsets=[0, 32]) == -1                       # a power of two above the node count
    assert _call(lib, M=0, res=[[3, 3, 3]], offsets=[0, 0]) == -1 and _call(lib, M=0, res=[[3, 3, 3]], offsets=[5, 2]) == -1
    assert _call(lib, M=0, res=[[3, 3, 3]], offsets=[-1, 26]) == -1
    for size in (27, 16, 1):
        assert _call(lib, M=0, res=[[3, 3, 3]], offsets=[7, 7 + size]) == 0
    many = [[2, 2, 2]] * 33
    assert _call(lib, M=0, res=many, offsets=list(range(0, 8 * 34, 8))) == -1             # more than 32 levels
    assert _call(lib, M=0, res=many[:32], offsets=list(range(0, 8 * 33, 8))) == 0
    assert _call(lib, M=(1 << 31) // 8 + 1) == -2                                        # M * L * F >= 2^31
    assert _call(lib, M=0, res=[[65536, 32768, 2]], offsets=[0, 16]) == -2               # Rx Ry >= 2^31
    for F, addr in ((2, 4), (4, 8), (8, 8), (8, 4), (1, 2)):                             # a misaligned table / grad_out is refused
        assert _call(lib, F=F, addr=addr) == -1, (F, addr)
    from directvoxgo_amd import _lib
    with pytest.raises(RuntimeError, match='invalid argument'):               # the typed call turns the code into an error
        _lib.call('dvgo_hash_bwd_xyz', None, 3, 1, None, None, None, None, None, None, 8, None, None)


def test_ops_reject_cpu_tensors():
    from directvoxgo_amd.ops import HashLevels, hash_bwd_xyz, hash_sample
    xyz, mn, mx = torch.zeros(7, 3, requires_grad=True), -torch.ones(3), torch.ones(3)
    table = torch.zeros(int(OFFSETS[-1]), 2)
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        hash_sample(table, xyz, mn, mx, RES, OFFSETS, position_grad=True)
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        hash_bwd_xyz(table, torch.zeros(7, 8), xyz.detach(), mn, mx, HashLevels(RES, OFFSETS))


# ---------------------------------------------------------------------------------------------- model and pose, host side
BASE = dict(num_voxels=10 * 12 * 14, num_voxels_base=16 ** 3, alpha_init=1e-2, fast_color_thres=1e-4)
BOX = ([-1.0, -1.2, -1.4], [1.0, 1.2, 1.4])
SMALL = dict(n_levels=4, n_feat=2, log2_hashmap_size=10, base_res=4, max_res=32, rgbnet_width=64)
RK = dict(near=0.1, far=1.0, stepsize=0.5, bg=1)


def _model(**kw):
    from directvoxgo_amd.hashgrid import HashVoxGO
    return HashVoxGO(*BOX, **{**BASE, **SMALL, **kw})


def test_raygrad_is_a_plain_attribute_and_survives_load_model(tmp_path):
    from directvoxgo_amd.checkpoint import load_model, save_checkpoint
    from directvoxgo_amd.hashgrid import HashVoxGO
    assert _model().raygrad is False and _model(raygrad=True).raygrad is True and _model(raygrad=1).raygrad is True
    m = _model(raygrad=True)
    kw = m.get_kwargs()
    assert 'raygrad' not in kw and set(kw) == set(_model().get_kwargs()) and not any('raygrad' in k for k in m.state_dict())
    path = str(tmp_path / 'h.tar')
    save_checkpoint(path, m, None, 3)
    assert load_model(HashVoxGO, path).raygrad is False
    m2 = load_model(HashVoxGO, path, raygrad=True)
    assert m2.raygrad is True and set(m2.state_dict()) == set(m.state_dict()) and torch.equal(m2.hash_table, m.hash_table)


def test_refine_poses_accepts_only_the_model_with_raygrad():
    from directvoxgo_amd.hashgrid import HASH_FINE_TRAIN
    from directvoxgo_amd.pose import CameraRefiner, _supported, refine_poses
    H = W = 4
    K = np.array([[4.0, 0, 2], [0, 4.0, 2], [0, 0, 1]], np.float32)
    ref = CameraRefiner(np.eye(4, dtype=np.float32)[None, :3], [[H, W]], [K])
    args = (ref, torch.zeros(1, H, W, 3), HASH_FINE_TRAIN, RK, 1, 8, 1e-3)
    assert not _supported(_model()) and not _supported(_model(fused=False))
    assert _supported(_model(raygrad=True)) and _supported(_model(raygrad=True, fused=False))
    with pytest.raises(NotImplementedError, match='refine_poses: HashVoxGO.*construct it with raygrad=True'):
        refine_poses(_model(), *args)
    for m in (_model(raygrad=True), _model(raygrad=True, fused=False)):                # before fused_raygrad is touched
        with pytest.raises(ValueError, match='HashVoxGO.*op-by-op path only'):
            refine_poses(m, *args, fused=True)
        assert 'fused_raygrad' not in m.__dict__
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):                   # accepted: the render is reached
        refine_poses(_model(raygrad=True), *args)


def test_rays_without_grad_and_models_without_the_option_keep_their_path(monkeypatch):
    """forward takes _forward_raygrad only with the option, grad mode and rays that require grad."""
    from directvoxgo_amd.hashgrid import HashVoxGO
    seen = []
    monkeypatch.setattr(HashVoxGO, '_forward_raygrad', lambda self, *a, **k: seen.append('raygrad'))
    monkeypatch.setattr(HashVoxGO, 'render', lambda self, *a, **k: seen.append('render'))
    o, d = torch.zeros(4, 3), torch.ones(4, 3)
    og = torch.zeros(4, 3, requires_grad=True)
    _model(raygrad=True)(og, d, d, **RK)
    _model(raygrad=True, fused=False)(o, d.clone().requires_grad_(), d, **RK)
    _model(raygrad=True)(o, d, d, **RK)
    with torch.no_grad():
        _model(raygrad=True)(og, d, d, **RK)
    _model()(og, d, d, **RK)
    assert seen == ['raygrad', 'raygrad', 'render', 'render', 'render']
