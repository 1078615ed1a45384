"""GPU: ray gradients through the grid sampler, from the kernel to pose refinement.

  dvgo_grid_sample_bwd_xyz   every record inside tests/raygrad_oracle.py's bound on every dispatch branch (channel-first,
                             channels-last float4, the same tensor misaligned by one float, channels-last C = 3, odd C, an
                             axis of size 1) at M in {0, 1, 257}: interior points, lattice planes, the six faces, padded
                             corners, and exact zeros more than one cell outside; grad_xyz pre-filled with NaN
  ops.grid_sample            with xyz.requires_grad the grid gradient keeps its bits; without it nothing changes
  ops.ray_points             forward bit for bit; grad_o / grad_d inside tests/grid_oracle.py's segment-sum bound, empty
                             rays exact zeros
  DirectVoxGO.forward        with rays that require grad: the dict of the fused=False forward bit for bit, rays_o.grad and
                             rays_d.grad against a float64 torch-CPU restatement of the same graph (tolerance: 4 x the
                             float32 CPU evaluation's own error, measured in the test)
  pose.refine_poses          a perturbed 6-view capture of a frozen model comes back: loss, rotation and translation error
                             of every view below their initial values; with train_model both grids and delta get gradients
The worst err / bound per kernel case is printed when the module finishes (pytest -s): information, never a threshold.
"""
import copy
import math

import numpy as np
import pytest
import torch

import grid_oracle as G
import raygrad_oracle as R

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print(f'\n{k}: {WORST[k]}', end='')
    print()


@pytest.fixture(scope='module')
def L():
    from directvoxgo_amd import _lib
    return _lib


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = host(a) if isinstance(a, torch.Tensor) else a, host(b) if isinstance(b, torch.Tensor) else b
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def in_layout(grid_np, layout, offset=0):
    """[C,X,Y,Z] numpy -> [1,C,X,Y,Z] on the device, channel-first or channels-last, its base `offset` floats into a buffer"""
    C, X, Y, Z = grid_np.shape
    n = C * X * Y * Z
    buf = torch.zeros(n + offset, dtype=torch.float32, device='cuda')
    strides = (n, 1, Y * Z * C, Z * C, C) if layout == 'cl' else (n, X * Y * Z, Y * Z, Z, 1)
    g = torch.as_strided(buf, (1, C, X, Y, Z), strides, storage_offset=offset)
    g.copy_(cu(grid_np)[None])
    assert g.data_ptr() % 16 == (4 * offset) % 16
    return g


# ------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize('M', R.SAMPLE_COUNTS)
@pytest.mark.parametrize('C,layout,dims,offset', R.GRIDS, ids=lambda v: str(v).replace(' ', ''))
def test_kernel_inside_the_oracle_bound(L, C, layout, dims, offset, M):
    X, Y, Z = dims
    grid_np = R.grid_values(C, dims, 21)
    grid = in_layout(grid_np, layout, offset)
    _, sC, sX, sY, sZ = grid.stride()
    mn, mx = cu(R.MN), cu(R.MX)
    xyz_np, gout_np = R.points(dims, M, seed=22), R.grad_values(M, C, 23)
    xyz, gout = cu(xyz_np.reshape(M, 3)), cu(gout_np.reshape(M, C))
    out = torch.full((max(M, 1), 3), float('nan'), device='cuda')
    L.call('dvgo_grid_sample_bwd_xyz', grid, C, X, Y, Z, sC, sX, sY, sZ, gout, xyz, mn, mx, M, out, L.stream_of(out))
    got = host(out)
    if M == 0:
        assert np.all(np.isnan(got))                         # no launch, nothing written
        return
    I = R.inputs32(xyz_np, R.MN, R.MX, dims)
    S = R.sums(grid_np, gout_np, I, R.scale(R.MN, R.MX, dims))
    if M == 257 and min(dims) > 1:                           # the point families are all there
        nin = I.inb.sum(-1)
        assert (nin == 8).sum() > 60 and ((nin > 0) & (nin < 8)).sum() > 30 and (nin == 0).sum() >= 32
        assert np.all(S.mag[nin == 0] == 0)
    r = R.check(S, got, what=f'bwd_xyz C={C} {layout} {dims} +{offset}')
    key = f'worst err / bound  bwd_xyz C={C} {layout} {dims} +{offset}'
    WORST[key] = max(WORST.get(key, 0.0), r)


# ------------------------------------------------------------------------------------------ ops.grid_sample
NODE_DIMS = (5, 3, 9)                                        # size - 1 a power of two: node positions are exact


def _nodes():
    mn, mx = np.zeros(3, np.float32), np.array(NODE_DIMS, np.float32) - 1
    ijk = np.stack(np.meshgrid(*[np.arange(n) for n in NODE_DIMS], indexing='ij'), -1).reshape(-1, 3)
    return mn, mx, ijk.astype(np.float32)


@pytest.mark.parametrize('C,layout', [(1, 'cf'), (12, 'cl'), (3, 'cl'), (5, 'cf')])
def test_grid_sample_grid_gradient_keeps_its_bits(C, layout):
    """one sample per voxel, on the node: every voxel receives one non-zero term, so the atomics' order cannot matter"""
    from directvoxgo_amd import ops
    mn, mx, xyz_np = _nodes()
    M = xyz_np.shape[0]
    I = R.inputs32(xyz_np, mn, mx, NODE_DIMS)
    assert np.all((I.w == 0) | (I.w == 1))
    grid_np, gout = R.grid_values(C, NODE_DIMS, 31), cu(R.grad_values(M, C, 32))
    res = {}
    for need in (False, True):
        g = in_layout(grid_np, layout).requires_grad_()
        x = cu(xyz_np).requires_grad_(need)
        out = ops.grid_sample(g, x, cu(mn), cu(mx))
        out.reshape(M, C).backward(gout)
        res[need] = (out.detach(), g.grad, x.grad)
    assert same_bits(res[False][0], res[True][0]) and same_bits(res[False][1], res[True][1])
    assert res[False][1].stride() == res[True][1].stride()
    assert res[False][2] is None and res[True][2] is not None
    S = R.sums(grid_np, host(gout), I, R.scale(mn, mx, NODE_DIMS))
    R.check(S, host(res[True][2]), what=f'ops.grid_sample xyz.grad C={C} {layout}')
    assert same_bits(res[True][0].reshape(M, C), np.moveaxis(grid_np.reshape(C, -1), 0, -1))   # on the nodes: the values


def test_grid_sample_without_position_gradient_saves_what_it_saved():
    from directvoxgo_amd import ops
    mn, mx, xyz_np = _nodes()
    g = in_layout(R.grid_values(3, NODE_DIMS, 33), 'cl').requires_grad_()
    x, tmn, tmx = cu(xyz_np), cu(mn), cu(mx)
    out = ops._GridSample.apply(g, x, tmn, tmx)
    assert len(out.grad_fn.saved_tensors) == 3
    out2 = ops._GridSample.apply(g, x.clone().requires_grad_(), tmn, tmx)
    assert len(out2.grad_fn.saved_tensors) == 4 and same_bits(out, out2)
    assert same_bits(out, ops.grid_sample(g, x, tmn, tmx))
    with torch.no_grad():
        assert same_bits(out, ops.grid_sample(g, x.clone().requires_grad_(), cu(mn), cu(mx)))


# ------------------------------------------------------------------------------------------ ops.ray_points
def test_ray_points_sums_per_ray():
    from directvoxgo_amd import ops
    counts = [0, 1, 3, 70, 0]                                # 70 crosses a wavefront of segment_sum
    N, M = len(counts), sum(counts)
    rng = np.random.default_rng(41)
    ray_id = np.repeat(np.arange(N), counts).astype(np.int64)
    o, d = rng.standard_normal((N, 3)).astype(np.float32), rng.standard_normal((N, 3)).astype(np.float32)
    lam = rng.uniform(0.5, 6.0, M).astype(np.float32)
    pts = rng.standard_normal((M, 3)).astype(np.float32)    # (whatever the sampler wrote: the forward hands it through)
    g = rng.standard_normal((M, 3)).astype(np.float32)
    to, td = cu(o).requires_grad_(), cu(d).requires_grad_()
    tp = cu(pts)
    out = ops.ray_points(to, td, cu(lam), cu(ray_id), tp)
    assert same_bits(out, pts) and out.data_ptr() != tp.data_ptr() and out.requires_grad
    out.backward(cu(g))
    zeros = np.zeros((N, 3), np.float32)
    for name, got, src in (('grad_o', to.grad, g), ('grad_d', td.grad, lam[:, None] * g)):
        assert src.dtype == np.float32
        S = G.segment_sums(src, ray_id, zeros)
        r = G.check_segment(S, host(got), zeros, what=f'ray_points {name}')
        WORST[f'worst err / bound  ray_points {name}'] = r
        assert np.all(host(got)[[0, 4]] == 0)
    only_d = cu(d).requires_grad_()
    ops.ray_points(cu(o), only_d, cu(lam), cu(ray_id), tp).backward(cu(g))
    assert same_bits(only_d.grad, td.grad)
    empty = ops.ray_points(to, td, cu(lam[:0]), cu(ray_id[:0]), tp[:0])
    (ge, _) = torch.autograd.grad(empty.sum(), (to, td), allow_unused=True)
    assert ge.shape == (N, 3) and float(ge.abs().sum()) == 0


# ------------------------------------------------------------------------------------------ end to end
RK = dict(near=2.0, far=6.0, stepsize=0.5, bg=1, render_depth=True)
HALF = 1.5 * 1.05


def make_model(rgbnet_dim, world, seed, capture=False):
    """A small DirectVoxGO on the device with its occupancy mask from the density.  Default: scenes.blob_density and random
    features.  `capture`: a scene to register cameras against -- five small blobs at different depths (so that a sideways
    move of a camera and a turn of it differ by parallax: one centred ball leaves the orbit about it nearly unobservable) with
    a saturated, position-dependent colour each."""
    from directvoxgo_amd import scenes
    from directvoxgo_amd.dvgo import DirectVoxGO
    gen = torch.Generator().manual_seed(seed)
    mn, mx = torch.full((3,), -HALF), torch.full((3,), HALF)
    kw = dict(num_voxels=world ** 3, num_voxels_base=world ** 3, alpha_init=1e-2, fast_color_thres=1e-4)
    if rgbnet_dim:
        kw.update(rgbnet_dim=rgbnet_dim, rgbnet_width=128)
    torch.manual_seed(seed)
    m = DirectVoxGO(mn, mx, **kw)
    ws = tuple(int(v) for v in m.world_size)
    if capture:
        x, y, z = torch.meshgrid(*[torch.linspace(-HALF, HALF, n) for n in ws], indexing='ij')
        centres = torch.tensor([[0.6, 0.1, -0.3], [-0.5, 0.5, 0.2], [0.0, -0.7, 0.4], [-0.3, -0.2, -0.7], [0.4, 0.6, 0.6]])
        r4 = torch.stack([((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) / 0.4 ** 2 for c in centres]).pow(2)
        density = 16.0 * torch.exp(-r4).amax(0) - 9.0
        k0 = torch.stack([3 * torch.sin(3 * x + 2 * y), 3 * torch.sin(3 * y - 2 * z + 1), 3 * torch.sin(3 * z + 2 * x + 2)])[None]
    else:
        density = scenes.blob_density(ws, mn, mx, gen)
        k0 = torch.randn((1, m.k0_dim, *ws), generator=gen) * 0.3
    alpha = torch.nn.functional.max_pool3d(scenes.activate(density, m.act_shift, 1.0)[None, None], 3, 1, 1)[0, 0]
    with torch.no_grad():
        m.density.copy_(density[None, None])
        m.k0.copy_(k0)
        m.mask_cache.mask.copy_(alpha > 1e-4)
    m = m.cuda()
    assert m.mask_cache is not None and 0.02 < float(m.mask_cache.mask.float().mean()) < 0.98
    return m


@pytest.fixture(scope='module', params=[0, 12], ids=['colour-grid', 'fused-head'])
def scene(request):
    from directvoxgo_amd import scenes
    m = make_model(request.param, 20, seed=3)
    o, d, v = scenes.camera_rays(8, 12, 13.0, scenes.pose_spherical(30.0, -30.0, 4.0))
    assert o.shape == (96, 3)
    return m, o.cuda(), d.cuda(), v.cuda()


def _dict_bits_equal(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert same_bits(a[k], b[k]), k


def test_forward_values_are_the_unfused_forward(scene):
    m, o, d, v = scene
    assert m.fused and (m.rgbnet is None or m.k0.stride(1) == 1)
    try:
        m.fused = False
        with torch.no_grad():
            plain = m(o, d, v, **RK)
        assert plain['ray_id'].numel() > 300
        res = m(o.clone().requires_grad_(), d.clone().requires_grad_(), v, **RK)
        assert res['rgb_marched'].requires_grad
        _dict_bits_equal(plain, res)
        with torch.no_grad():                                # no grad mode, or rays that do not ask: today's path
            _dict_bits_equal(plain, m(o.clone().requires_grad_(), d, v, **RK))
        only_d = m(o, d.clone().requires_grad_(), v, **RK)
        _dict_bits_equal(plain, only_d)
    finally:
        m.fused = True
    # fused = True: the same op sequence with the model's own (fused) colour head
    res = m(o.clone().requires_grad_(), d.clone().requires_grad_(), v, **RK)
    pts, ray_id, step_id = m.sample_ray(o, d, **RK)
    keep = m.mask_cache(pts)
    want = m._forward_unfused(len(o), v, RK['stepsize'], RK['bg'], True, pts[keep], ray_id[keep], step_id[keep])
    _dict_bits_equal(want, res)
    if m.rgbnet is None:
        _dict_bits_equal(plain, res)


def _device_record(m, o, d):
    """What the float64 restatement takes from the device run: the kept-sample sets, the cells and lam."""
    from directvoxgo_amd import render_utils
    from directvoxgo_amd.ops import Alphas2Weights
    with torch.no_grad():
        stepdist = RK['stepsize'] * m.voxel_size
        pts, out, ray_id, step_id, _, t_min, _ = render_utils.sample_pts_on_rays(o, d, m.xyz_min, m.xyz_max, RK['near'], RK['far'], stepdist)
        keep = ~out
        pts, ray_id, step_id = pts[keep], ray_id[keep], step_id[keep]
        keep = m.mask_cache(pts)
        pts, ray_id, step_id = pts[keep], ray_id[keep], step_id[keep]
        lam = t_min[ray_id] + (float(stepdist) * step_id) / d.norm(dim=-1)[ray_id]
        alpha = m.activate_density(m.grid_sampler(pts, m.density), RK['stepsize'] * m.voxel_size_ratio)
        m1 = alpha > m.fast_color_thres
        w1, _ = Alphas2Weights.apply(alpha[m1].contiguous(), ray_id[m1].contiguous(), len(o))
        m2 = w1 > m.fast_color_thres
    ws = tuple(int(x) for x in m.density.shape[2:])
    I = R.inputs32(host(pts), host(m.xyz_min), host(m.xyz_max), ws)
    rec = dict(ray_id0=ray_id.cpu(), lam=lam.cpu(), m1=m1.cpu(), act1=(w1 != 0).cpu(), m2=m2.cpu(), pts=pts.cpu(),
               ijk0=torch.from_numpy(I.ijk0), inb=torch.from_numpy(I.inb), ws=ws)
    return rec


def _trilinear(grid, pts, ijk0, inb, mn, mx):
    """grid [C,X,Y,Z], the cell fixed (ijk0, inb from the device's float32 positions), the weights from g in grid's dtype"""
    size = torch.tensor(grid.shape[1:], dtype=grid.dtype)
    g = (pts - mn) / (mx - mn) * (size - 1)
    w1 = g - ijk0.to(grid.dtype)
    w = torch.stack([1 - w1, w1], -1)                        # [M,3,2]
    out = torch.zeros(pts.shape[0], grid.shape[0], dtype=grid.dtype)
    for n in range(8):
        b = ((n >> 2) & 1, (n >> 1) & 1, n & 1)
        idx = [(ijk0[:, a] + b[a]).clamp(0, grid.shape[1 + a] - 1) for a in range(3)]
        v = grid[:, idx[0], idx[1], idx[2]].t()
        wn = (w[:, 2, b[2]] * w[:, 1, b[1]]) * w[:, 0, b[0]]
        out = out + torch.where(inb[:, n, None], wn[:, None] * v, torch.zeros_like(v))
    return out


def _restate(m, o, d, v, rec, dtype):
    """The graph of DirectVoxGO._forward_raygrad in torch on the CPU, in `dtype`, with its stop-gradients: lam, the kept
    sets, the cells and viewdirs are constants.  -> (d loss / d rays_o, d loss / d rays_d), loss = rgb_marched.square().sum()"""
    from directvoxgo_amd.voxel_model import _posenc
    N = o.shape[0]
    o = o.detach().cpu().to(dtype).requires_grad_()
    d = d.detach().cpu().to(dtype).requires_grad_()
    mn, mx = m.xyz_min.cpu().to(dtype), m.xyz_max.cpu().to(dtype)
    rid0 = rec['ray_id0']
    pts = o[rid0] + d[rid0] * rec['lam'].to(dtype)[:, None]
    dens = _trilinear(m.density.detach().cpu()[0].to(dtype), pts, rec['ijk0'], rec['inb'], mn, mx)[:, 0]
    interval = float(RK['stepsize'] * m.voxel_size_ratio)
    alpha = 1 - torch.pow(1 + torch.exp(dens + float(m.act_shift)), -interval)
    m1, m2, act = rec['m1'], rec['m2'], rec['act1']
    alpha1, rid1 = alpha[m1], rid0[m1]
    f = torch.where(act, 1 - alpha1 + 1e-10, torch.ones_like(alpha1))
    T, last = [], []
    for r in range(N):
        seg = f[rid1 == r]
        c = torch.cumprod(seg, 0)
        T.append(torch.cat([torch.ones(1, dtype=dtype), c[:-1]]) if len(seg) else seg)
        last.append(c[-1] if len(seg) else torch.ones((), dtype=dtype))
    w1 = torch.where(act, torch.cat(T) * alpha1, torch.zeros_like(alpha1))
    last = torch.stack(last)
    w2, rid2 = w1[m2], rid1[m2]
    k0 = _trilinear(m.k0.detach().cpu()[0].to(dtype), pts[m1][m2], rec['ijk0'][m1][m2], rec['inb'][m1][m2], mn, mx)
    if m.rgbnet is None:
        rgb = torch.sigmoid(k0)
    else:
        net = copy.deepcopy(m.rgbnet).cpu().to(dtype)
        emb = _posenc(v.detach().cpu().to(dtype), m.viewfreq.cpu().to(dtype))[rid2]
        rgb = torch.sigmoid(net(torch.cat([k0[:, 3:], emb], -1)) + k0[:, :3])
    marched = torch.zeros(N, 3, dtype=dtype).index_add(0, rid2, w2[:, None] * rgb) + last[:, None] * RK['bg']
    loss = marched.square().sum()
    go, gd = torch.autograd.grad(loss, (o, d))
    return go.double(), gd.double(), marched.detach().double()


def test_ray_gradients_match_the_float64_restatement(scene):
    m, o, d, v = scene
    ro, rd = o.clone().requires_grad_(), d.clone().requires_grad_()
    res = m(ro, rd, v, **RK)
    res['rgb_marched'].square().sum().backward()
    assert ro.grad is not None and rd.grad is not None
    rec = _device_record(m, o, d)
    assert same_bits(rec['ray_id0'][rec['m1']][rec['m2']], res['ray_id'])         # the record is this forward's
    o64, d64, marched64 = _restate(m, o, d, v, rec, torch.float64)
    o32, d32, _ = _restate(m, o, d, v, rec, torch.float32)
    assert float((marched64 - res['rgb_marched'].detach().cpu().double()).abs().max()) < 1e-4   # (the restatement is this render)
    name = 'fused-head' if m.rgbnet is not None else 'colour-grid'
    for what, g64, g32, dev in (('rays_o.grad', o64, o32, ro.grad), ('rays_d.grad', d64, d32, rd.grad)):
        e32 = float((g32 - g64).abs().max())
        err = float((dev.detach().cpu().double() - g64).abs().max())
        print(f'\n{name} {what}: max |g64| {float(g64.abs().max()):.4g}  e32 {e32:.4g}  device error {err:.4g}  (allowed {4 * e32:.4g})', end='')
        WORST[f'end to end {name} {what}'] = f'e32 {e32:.4g}  device error {err:.4g}'
        assert float(g64.abs().max()) > 1e-3 and e32 > 0
        assert err <= 4 * e32, (what, err, e32)


# ------------------------------------------------------------------------------------------ wiring and signs
def _capture(n_views=6, hw=24, focal=30.0, radius=4.0, seed=7):
    from directvoxgo_amd import scenes
    from directvoxgo_amd.pose import se3_exp
    gen = torch.Generator().manual_seed(seed)
    true = torch.stack([scenes.pose_spherical(60.0 * i + 10.0, -30.0 - 5.0 * (i % 3), radius)[:3, :4] for i in range(n_views)])
    axis = torch.randn(n_views, 3, generator=gen)
    axis = axis / axis.norm(dim=-1, keepdim=True)
    shift = torch.randn(n_views, 3, generator=gen)
    shift = shift / shift.norm(dim=-1, keepdim=True) * (0.03 * radius)
    E = se3_exp(torch.cat([axis * math.radians(2.0), torch.zeros(n_views, 3)], -1))[:, :, :3]
    noisy = torch.cat([E @ true[:, :, :3], true[:, :, 3:] + shift[:, :, None]], -1)
    K = np.array([[focal, 0, 0.5 * hw], [0, focal, 0.5 * hw], [0, 0, 1]], np.float32)
    return true, noisy, np.array([[hw, hw]] * n_views), np.stack([K] * n_views)


def _pose_errors(est, true):
    """-> (rotation error [n] in radians, translation error [n])"""
    est, true = est.detach().cpu().double(), true.cpu().double()
    rel = est[:, :, :3] @ true[:, :, :3].transpose(1, 2)
    cos = ((rel.diagonal(dim1=1, dim2=2).sum(-1) - 1) / 2).clamp(-1, 1)
    return torch.acos(cos), (est[:, :, 3] - true[:, :, 3]).norm(dim=-1)


# Adam moves a parameter by about the step size per iteration while its gradient keeps its sign.  The correction a view needs
# is up to |t| * 2 deg + 3 % of the radius = 0.14 + 0.12 in delta's units (the update is a world-frame one: turning a camera
# about the origin carries its centre along), i.e. 65 iterations at 4e-3, which leaves two thirds of the 200 to settle.
LRATE_POSE = 4e-3


def _refine(m, seed=7, lrate_pose=LRATE_POSE, n_iters=200):
    """Ground truth from the true poses, then refine_poses from the perturbed ones on all pixels.
    -> (losses, rotation errors before / after, translation errors before / after, the capture)"""
    from directvoxgo_amd.pose import CameraRefiner, refine_poses
    from directvoxgo_amd.train import COARSE_TRAIN
    true, noisy, HW, Ks = _capture(seed=seed)
    n, hw = len(true), int(HW[0, 0])
    rk = dict(near=2.0, far=6.0, stepsize=0.5, bg=1)
    exact = CameraRefiner(true, HW, Ks).cuda()
    view = torch.arange(n, device='cuda').repeat_interleave(hw * hw)
    p = torch.arange(hw * hw, device='cuda').repeat(n)
    with torch.no_grad():
        o, d, v = exact.rays(view, p % hw, p // hw)
        images = m(o, d, v, **rk)['rgb_marched'].reshape(n, hw, hw, 3)
    assert float(images.std()) > 0.05                         # there is something to register against
    ref = CameraRefiner(noisy, HW, Ks).cuda()
    rot0, tr0 = _pose_errors(ref.poses(), true)
    cfg = dict(COARSE_TRAIN, weight_entropy_last=0.0, weight_rgbper=0.0)
    losses = refine_poses(m, ref, images, cfg, rk, n_iters=n_iters, n_rand=None, lrate_pose=lrate_pose)
    rot1, tr1 = _pose_errors(ref.poses(), true)
    return losses, rot0, rot1, tr0, tr1, (noisy, HW, Ks, images, rk)


def test_refine_poses_recovers_a_perturbed_capture():
    from directvoxgo_amd.pose import CameraRefiner, refine_poses
    from directvoxgo_amd.train import COARSE_TRAIN
    m = make_model(0, 24, seed=5, capture=True)
    for p in m.parameters():
        p.requires_grad_(False)
    losses, rot0, rot1, tr0, tr1, (noisy, HW, Ks, images, rk) = _refine(m)
    assert torch.allclose(rot0, torch.full_like(rot0, math.radians(2.0)), atol=1e-4) and torch.allclose(tr0, torch.full_like(tr0, 0.12), atol=1e-4)
    print(f'\nrefine_poses: loss {losses[0]:.3e} -> {losses[-1]:.3e}; rotation error (deg) {np.degrees(rot0.numpy()).round(3).tolist()} -> '
          f'{np.degrees(rot1.numpy()).round(3).tolist()}; translation error {tr0.numpy().round(4).tolist()} -> {tr1.numpy().round(4).tolist()}', end='')
    WORST['refine_poses'] = (f'loss {losses[0]:.3e} -> {losses[-1]:.3e}, worst rotation error {math.degrees(float(rot1.max())):.3f} deg (from 2), '
                             f'worst translation error {float(tr1.max()):.4f} (from 0.12)')
    assert len(losses) == 200 and all(math.isfinite(x) for x in losses)
    assert losses[-1] < losses[0]
    assert bool((rot1 < rot0).all()) and bool((tr1 < tr0).all())
    assert all(q.grad is None for q in m.parameters())       # a frozen model is left alone

    # poses and model together: both receive gradients in the same iteration
    m2 = make_model(0, 24, seed=5, capture=True)
    ref2 = CameraRefiner(noisy, HW, Ks).cuda()
    before = m2.density.detach().clone()
    losses2 = refine_poses(m2, ref2, images, dict(COARSE_TRAIN), rk, n_iters=20, n_rand=1024, lrate_pose=LRATE_POSE, train_model=True, seed=1)
    assert len(losses2) == 20 and all(math.isfinite(x) for x in losses2)
    for g in (m2.density.grad, m2.k0.grad, ref2.delta.grad):
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().sum()) > 0
    assert not torch.equal(before, m2.density.detach()) and float(ref2.delta.detach().abs().sum()) > 0
