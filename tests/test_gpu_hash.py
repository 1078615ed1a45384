"""GPU: the hash-grid sampler (csrc/hashgrid.hip) against the float64 oracle of tests/hash_oracle.py on every output and
every table element; its tie to ops.grid_sample on a dense level; the op's autograd against a float64 torch restatement; and
HashVoxGO fused against unfused, through the training step, a checkpoint, scale_volume_grid and render_viewpoints.

Error bounds (gamma, SLACK and TINY of tests/brick_oracle.py; A = the magnitude the oracle returns), derived, not tuned:
  forward   |got - ref| <= gamma(10 + SLACK) A + TINY: two roundings in the corner weight and eight in the fma chain.
  backward  |got - ref| <= gamma(n + 3 + SLACK) A + TINY per table element of a row with n contributions: the weight, the
            product, and n - 1 additions in any order -- of the atomics and of a lane's own run sums alike: the sums of a
            run and the atomics that deliver them form one summation tree over the same n terms.
  An element nobody touches is exactly 0.  No sample and no element is excluded from either check.
"""
import functools

import numpy as np
import pytest
import torch

import hash_oracle as HO

pytestmark = pytest.mark.gpu

MN, MX = np.array([-1.0, -0.8, -0.6], np.float32), np.array([0.9, 1.1, 0.7], np.float32)
# one table mixing levels: dense, dense, hashed into 16 rows (collisions, same-cell ones included), hashed into 2^10
RES = np.array([[2, 2, 2], [2, 3, 7], [9, 9, 9], [33, 17, 40]], np.int32)
OFFSETS = np.cumsum([0, 8, 42, 16, 1024]).astype(np.int64)
T = int(OFFSETS[-1])
MS = (0, 1, 63, 64, 65, 4099)
FS = (1, 2, 4, 8)
RUNS = (0, 1, 3, 8)                        # modes 1 and 3: the default (32), nothing merged, a length that divides nothing here, 8
RUN_LEN, N_RUNS = 40, 20


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _runs(rng, n):
    """n runs of RUN_LEN consecutive points along a line, 0.3 of the finest level's cell apart: [n * RUN_LEN, 3]."""
    cell = ((MX - MN) / (RES[-1] - 1)).min()
    out = []
    for _ in range(n):
        start = MN + (MX - MN) * rng.random(3)
        d = rng.standard_normal(3); d /= np.linalg.norm(d)
        out.append(start + np.arange(RUN_LEN)[:, None] * (0.3 * cell * d))
    return np.concatenate(out).astype(np.float32)


def points(M, rng):
    """In this order, cut to M: the box's two corners; four points on lattice planes of every level (two of their three
    coordinates on a node); runs of consecutive points; the same runs with their rows shuffled; random points up to 10 % of
    the box outside it; and, where M has room, one more run that ends at M."""
    special = [MN, MX]
    for R in RES:
        for i in range(4):
            p = MN + (MX - MN) * rng.random(3)
            for a in ((i + 1) % 3, (i + 2) % 3):
                p[a] = MN[a] + (MX[a] - MN[a]) * np.float32(int(rng.integers(R[a])) / (R[a] - 1))
            special.append(p)
    runs = _runs(rng, N_RUNS)
    xyz = np.concatenate([np.array(special), runs, runs[rng.permutation(len(runs))],
                          MN + (MX - MN) * (rng.random((M, 3)) * 1.2 - 0.1)]).astype(np.float32)[:M]
    if M >= 4 * RUN_LEN:
        xyz[M - RUN_LEN:] = _runs(rng, 1)
    return xyz


@functools.lru_cache(maxsize=None)
def case(F):
    """Inputs and oracle results for F floats per row: the table and, per M, (xyz, forward value and A, grad_out, backward
    reference).  Computed once, shared, never written to."""
    rng = np.random.default_rng(200 + F)
    table = rng.standard_normal((T, F)).astype(np.float32)
    per_m = {}
    for M in MS:
        xyz = points(M, rng)
        val, A = HO.forward(table, xyz, MN, MX, RES, OFFSETS)
        gout = rng.standard_normal((M, len(RES) * F)).astype(np.float32)
        per_m[M] = (xyz, val, A, gout, HO.backward((T, F), xyz, MN, MX, RES, OFFSETS, gout))
    return table, per_m


def test_points_cover_the_edge_cases():
    xyz = case(2)[1][4099][0]
    inside = ((xyz >= MN) & (xyz <= MX)).all(1)
    assert 100 < (~inside).sum() < 2000                                       # outside the box: clamped
    for l in range(len(RES)):
        rows, w, cell = HO.corners(RES, OFFSETS, l, xyz, MN, MX)
        assert ((w == 1).any(0)).sum() >= 2 and (w == 0).any()                # nodes exactly: the box's corners at least
        assert (cell.min(0) == 0).all() and (cell.max(0) == RES[l] - 2).all()     # the first and the last cell of every axis
        assert rows.min() >= OFFSETS[l] and rows.max() < OFFSETS[l + 1]
        same = (np.diff(cell[2 + 16:2 + 16 + N_RUNS * RUN_LEN].reshape(N_RUNS, RUN_LEN, 3), axis=1) == 0).all(2)
        if l < 3:
            assert same.mean() > 0.8                                          # a run mostly stays in its cell on coarse levels
        else:
            assert 0.2 < same.mean() < 0.95                                   # and changes it every few points on the finest
    assert HO.same_cell_collisions(RES, OFFSETS, 2, xyz, MN, MX) > 100        # two corners of ONE cell on one row
    assert HO.same_cell_collisions(RES, OFFSETS, 0, xyz, MN, MX) == HO.same_cell_collisions(RES, OFFSETS, 1, xyz, MN, MX) == 0
    n = case(2)[1][4099][4][2]
    assert (n[OFFSETS[2]:OFFSETS[3]] > 100).all()                             # 16 rows take every corner of the level
    assert (case(2)[1][65][4][2] == 0).any()                                  # rows nobody touches (the small cases)


def _check_bwd(got_t, ref, what, prefilled=None):
    g, Ag, n = ref
    got = got_t.cpu().numpy().astype(np.float64)
    if prefilled is not None:
        g, Ag = g + prefilled, Ag + np.abs(prefilled)
    err, bound = np.abs(got - g), HO.bwd_bound(Ag, n, 0 if prefilled is None else 1)
    assert (err <= bound).all(), (what, float((err - bound).max()), int((err > bound).sum()))
    if prefilled is None:
        assert (got[n == 0] == 0).all(), what
    return float((err / np.maximum(bound, 1e-300)).max())


@pytest.mark.parametrize('F', FS)
def test_sampler_against_oracle(F):
    from directvoxgo_amd.ops import HashLevels, hash_bwd, hash_fwd
    table, per_m = case(F)
    lv = HashLevels(RES, OFFSETS)
    dt, mn, mx = cu(table), cu(MN), cu(MX)
    worst_f = worst_b = 0.0
    for M in MS:
        xyz, val, A, gout, ref = per_m[M]
        dx, dg = cu(xyz).reshape(M, 3), cu(gout).reshape(M, len(RES) * F)
        got_t = hash_fwd(dt, dx, mn, mx, lv)
        got = got_t.cpu().numpy().astype(np.float64)
        assert got.shape == val.shape == (M, len(RES) * F)
        err, bound = np.abs(got - val), HO.fwd_bound(A)
        if M:
            worst_f = max(worst_f, float((err / bound).max()))
        assert (err <= bound).all(), (M, float((err - bound).max()))
        assert torch.equal(got_t, hash_fwd(dt, dx, mn, mx, lv))               # bitwise repeatable
        for mode, run in [(1, r) for r in RUNS] + [(3, r) for r in RUNS] + [(2, 0), (0, 0)]:
            grad = torch.zeros(T, F, device='cuda')
            hash_bwd(dg, grad, dx, mn, mx, lv, run=run, mode=mode)
            worst_b = max(worst_b, _check_bwd(grad, ref, (M, mode, run)))
    print(f'F={F}: worst forward err / bound {worst_f:.3f}, worst backward err / bound {worst_b:.3f}')


def test_bwd_accumulates_into_the_callers_buffer():
    """A buffer holding random values before the launch: afterwards every element is its old value plus the gradient, with
    one more addition in the bound; an element nobody touches keeps its bits."""
    from directvoxgo_amd.ops import HashLevels, hash_bwd
    F = 2
    _, per_m = case(F)
    pre = np.random.default_rng(9).standard_normal((T, F)).astype(np.float32)
    lv = HashLevels(RES, OFFSETS)
    for M in (65, 4099):
        xyz, _, _, gout, ref = per_m[M]
        for mode in (1, 2, 3):
            grad = cu(pre.copy())
            hash_bwd(cu(gout), grad, cu(xyz), cu(MN), cu(MX), lv, mode=mode)
            _check_bwd(grad, ref, ('prefilled', M, mode), prefilled=pre.astype(np.float64))
            assert np.array_equal(grad.cpu().numpy()[ref[2] == 0], pre[ref[2] == 0])
    assert (per_m[65][4][2] == 0).any()


def test_two_backward_launches_agree_within_twice_the_bound():
    """Float atomics: the two sums need not be bit-equal, and are not asserted to be."""
    from directvoxgo_amd.ops import HashLevels, hash_bwd
    F = 4
    _, per_m = case(F)
    xyz, _, _, gout, (g, Ag, n) = per_m[4099]
    lv = HashLevels(RES, OFFSETS)
    a, b = torch.zeros(T, F, device='cuda'), torch.zeros(T, F, device='cuda')
    hash_bwd(cu(gout), a, cu(xyz), cu(MN), cu(MX), lv)
    hash_bwd(cu(gout), b, cu(xyz), cu(MN), cu(MX), lv)
    diff = np.abs(a.cpu().numpy().astype(np.float64) - b.cpu().numpy().astype(np.float64))
    assert (diff <= 2 * HO.bwd_bound(Ag, n)).all() and float(a.abs().sum()) > 0
    print('elements that differ between two launches:', int((diff > 0).sum()), 'of', diff.size)


def test_a_dense_level_is_grid_sample():
    """One dense level of res = dims, F = 1, against ops.grid_sample of the same values as [1,1,X,Y,Z], inside the box (where
    zero padding and the clamp state the same interpolant), within the forward bound."""
    from directvoxgo_amd.ops import grid_sample, hash_sample
    rng = np.random.default_rng(31)
    dims = (7, 9, 11)
    res, off = np.array([dims], np.int32), np.array([0, 7 * 9 * 11], np.int64)
    table = rng.standard_normal((off[1], 1)).astype(np.float32)
    xyz = (MN + (MX - MN) * rng.random((3000, 3))).astype(np.float32)
    xyz[:2] = MN, MX
    for a in range(3):                                                         # lattice planes of every axis
        xyz[2 + 10 * a:12 + 10 * a, a] = MN[a] + (MX[a] - MN[a]) * (rng.integers(dims[a], size=10) / np.float32(dims[a] - 1))
    val, A = HO.forward(table, xyz, MN, MX, res, off)
    got = hash_sample(cu(table), cu(xyz), cu(MN), cu(MX), res, off)
    ref = grid_sample(cu(table).reshape(1, 1, *dims), cu(xyz), cu(MN), cu(MX))
    assert got.shape == (3000, 1) and ref.shape == (3000,)
    err = np.abs(got[:, 0].cpu().numpy().astype(np.float64) - ref.cpu().numpy().astype(np.float64))
    bound = HO.fwd_bound(A[:, 0])
    print('worst |hash - grid_sample| / bound:', float((err / bound).max()))
    assert (err <= bound).all()
    assert (np.abs(got.cpu().numpy() - val) <= HO.fwd_bound(A)).all()


def _torch_restatement(table, xyz, mn, mx, res, off):
    """The same function in torch ops, in the dtype of its inputs (float64 on the CPU here): every level expanded to a dense
    [1,F,X,Y,Z] array by looking each node up, then F.grid_sample (trilinear, align_corners=True).  Differentiable in
    `table`.  For points inside the box, where the padding is not reached."""
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


@pytest.mark.parametrize('wants', [True, False])
def test_op_autograd_against_the_float64_restatement(wants):
    """ops.hash_sample against the float64 restatement on the CPU, at section 6's tolerances for this kind of comparison:
    values rtol 1e-5 / atol 1e-6, gradients rtol 1e-4 / atol 1e-6.  Box [-1, 1]^3, node counts 2^k + 1 and points on multiples
    of 2^-10 inside it: every float32 coordinate operation of the kernel is then exact, so the float64 evaluation sees the
    same cells and weights.  A table that wants no gradient gets none; xyz never gets one."""
    from directvoxgo_amd.ops import hash_sample
    rng = np.random.default_rng(41)
    mn, mx = np.float32([-1, -1, -1]), np.float32([1, 1, 1])
    res = np.array([[3, 5, 9], [17, 9, 33]], np.int32)
    off = np.array([0, 135, 135 + 256], np.int64)
    Fc, M = 2, 300
    table = (0.5 * rng.standard_normal((int(off[-1]), Fc))).astype(np.float32)
    xyz = (rng.integers(-1024, 1025, (M, 3)) / 1024.0).astype(np.float32)
    gout = rng.standard_normal((M, 2 * Fc)).astype(np.float32)
    t64 = torch.from_numpy(table).double().requires_grad_(True)
    ref = _torch_restatement(t64, torch.from_numpy(xyz).double(), torch.from_numpy(mn).double(), torch.from_numpy(mx).double(),
                             res, off)
    ref.backward(torch.from_numpy(gout).double())
    dt = cu(table).requires_grad_(wants)
    dx = cu(xyz).requires_grad_(True)
    out = hash_sample(dt, dx, cu(mn), cu(mx), torch.from_numpy(res), torch.from_numpy(off))
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), rtol=1e-5, atol=1e-6)
    assert out.requires_grad == wants
    if wants:
        out.backward(cu(gout))
        assert dt.grad.shape == dt.shape and float(dt.grad.abs().sum()) > 0
        np.testing.assert_allclose(dt.grad.cpu().numpy(), t64.grad.numpy(), rtol=1e-4, atol=1e-6)
    assert dx.grad is None
    shaped = hash_sample(dt, cu(xyz).reshape(15, 20, 3), cu(mn), cu(mx), res, off)
    assert shaped.shape == (15, 20, 2 * Fc) and torch.equal(shaped.reshape(M, -1), out)
    with pytest.raises(ValueError, match='power of two'):
        hash_sample(dt, dx, cu(mn), cu(mx), res, np.array([0, 135, 135 + 100]))


# ---------------------------------------------------------------------------------------------- the model
HASH = dict(n_levels=4, n_feat=2, log2_hashmap_size=10, base_res=8, max_res=64)


@pytest.fixture(scope='module')
def scene():
    from directvoxgo_amd.scenes import synthetic_scene
    return synthetic_scene(world=32, n_rays=256, seed=6, device='cuda')


def _scene_model(sc, fused=True, seed=1, **kw):
    from directvoxgo_amd.hashgrid import HashVoxGO
    torch.manual_seed(seed)
    m = HashVoxGO(sc['xyz_min'], sc['xyz_max'], **{**dict(
        num_voxels=sc['world'] ** 3, num_voxels_base=sc['world'] ** 3, alpha_init=1e-2, fast_color_thres=1e-4,
        rgbnet_width=64, fused=fused), **HASH, **kw})
    for p in m.rgbnet.parameters():
        torch.nn.init.normal_(p, std=0.1)
    with torch.no_grad():
        m.hash_table.normal_(std=0.3)                 # (the initialisation proper is 1e-4: features too small to tell paths apart)
    m = m.cuda()
    with torch.no_grad():
        m.density.copy_(sc['density']); m.mask_cache.mask.copy_(sc['mask'])
    return m


def test_fused_equals_unfused(scene):
    """Both paths call the same sampler on bit-equal positions and end in the same per-ray sum: with the same colour head
    (torch's) behind them the result dicts are equal bit for bit, key by key."""
    sc = scene
    ro, rd, vd = sc['rays_o'], sc['rays_d'], sc['viewdirs']
    rk = dict(near=sc['near'], far=sc['far'], bg=1, stepsize=0.5, render_depth=True)
    outs = {}
    for fused in (True, False):
        m = _scene_model(sc, fused=fused)
        assert m.levels.hashed == [False, True, True, True]
        m.fused_shade = False
        with torch.no_grad():
            outs[fused] = m(ro, rd, vd, **rk)
    a, b = outs[True], outs[False]
    assert set(a) == set(b) >= {'alphainv_last', 'weights', 'rgb_marched', 'raw_alpha', 'raw_rgb', 'ray_id', 'depth'}
    assert a['ray_id'].shape[0] > 256 and float((a['rgb_marched'] - 1).abs().max()) > 0.05
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_train_step_checkpoint_and_scale_volume_grid(scene, tmp_path):
    """Thirty TrainStep steps with HASH_FINE_TRAIN: finite, the loss falls, density, table and MLP move, and table rows whose
    gradient is zero in a step keep their value and both moments through it.  A checkpoint loaded into a fresh model gives
    equal state_dicts and an equal render.  scale_volume_grid resizes the density and leaves the table's bits alone."""
    from directvoxgo_amd.checkpoint import load_model, save_checkpoint
    from directvoxgo_amd.hashgrid import HASH_FINE_TRAIN, HashVoxGO
    from directvoxgo_amd.train import TrainStep
    sc = scene
    rk = dict(near=sc['near'], far=sc['far'], bg=1, stepsize=0.5)
    m = _scene_model(sc)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    step = TrainStep(m, dict(HASH_FINE_TRAIN), rk)
    assert not step.can_capture()
    args = (sc['rays_o'], sc['rays_d'], sc['viewdirs'], sc['target'])
    losses = [float(step(*args, global_step=s)) for s in range(1, 30)]
    st = step.optimizer.state[m.hash_table]
    held = [m.hash_table.detach().clone(), st['exp_avg'].clone(), st['exp_avg_sq'].clone()]
    losses.append(float(step(*args, global_step=30)))
    print('losses', losses[0], losses[-1])
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    g = m.hash_table.grad
    assert g is not None and g.shape == m.hash_table.shape and bool(torch.isfinite(g).all())
    zero, now = g == 0, [m.hash_table.detach(), st['exp_avg'], st['exp_avg_sq']]
    assert 0 < int(zero.sum()) < zero.numel()
    for was, is_ in zip(held, now):
        assert torch.equal(was[zero], is_[zero])
    assert not torch.equal(held[0][~zero], now[0][~zero]) and bool((now[2][~zero] > 0).all())
    after = m.state_dict()
    assert all(bool(torch.isfinite(v).all()) for v in after.values() if v.is_floating_point())
    for k in ('density', 'hash_table', 'rgbnet.0.weight', 'rgbnet.3.bias'):
        assert not torch.equal(before[k], after[k]), k
    path = str(tmp_path / 'hash.tar')
    save_checkpoint(path, m, step.optimizer, 30)
    m2 = load_model(HashVoxGO, path).cuda()
    assert m2.get_kwargs().keys() == m.get_kwargs().keys() and {k: m2.get_kwargs()[k] for k in HASH} == HASH
    assert set(m2.state_dict()) == set(after) and all(torch.equal(v, m2.state_dict()[k]) for k, v in after.items())
    with torch.no_grad():
        ra, rb = m(*args[:3], render_depth=True, **rk), m2(*args[:3], render_depth=True, **rk)
    assert all(torch.equal(ra[k], rb[k]) for k in ('rgb_marched', 'depth', 'weights', 'ray_id'))

    table = m.hash_table.detach().clone()
    levels = (m.levels.res, m.levels.offsets)
    m.scale_volume_grid(40 ** 3)
    ws = tuple(int(v) for v in m.world_size)
    assert min(ws) > 32 and tuple(m.density.shape[2:]) == ws and tuple(m.mask_cache.mask.shape) == ws
    assert torch.equal(m.hash_table.detach(), table) and (m.levels.res, m.levels.offsets) == levels
    res = m(*args[:3], **rk)
    assert res['ray_id'].shape[0] > 256 and bool(torch.isfinite(res['rgb_marched']).all())


def test_render_viewpoints_returns_the_models_own_render(scene):
    from directvoxgo_amd.render import get_rays_of_a_view, render_viewpoints
    from directvoxgo_amd.scenes import pose_spherical
    sc = scene
    m = _scene_model(sc)
    H = W = 16
    K = np.array([[20.0, 0, 0.5 * W], [0, 20.0, 0.5 * H], [0, 0, 1]], np.float32)
    poses = [pose_spherical(30.0, -30.0, 4.0), pose_spherical(-100.0, -20.0, 4.0)]
    rk = dict(near=sc['near'], far=sc['far'], bg=1, stepsize=0.5, inverse_y=False)
    rgbs, depths = render_viewpoints(m, [p.numpy() for p in poses], [(H, W)] * 2, [K] * 2, False, rk)
    assert rgbs.shape == (2, H, W, 3) and depths.shape == (2, H, W, 1)
    for i, pose in enumerate(poses):
        ro, rd, vd = get_rays_of_a_view(H, W, K, pose.cuda(), False, False, False, False)
        with torch.no_grad():
            res = m(ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous(), vd.reshape(-1, 3).contiguous(),
                    render_depth=True, **rk)
        assert float((res['rgb_marched'] - 1).abs().max()) > 0.05               # the view sees the object
        np.testing.assert_allclose(rgbs[i].reshape(-1, 3), res['rgb_marched'].cpu().numpy(), atol=1e-6)
        np.testing.assert_allclose(depths[i].reshape(-1), res['depth'].cpu().numpy(), atol=1e-4)
