"""GPU: the vector-matrix sampler (csrc/vm.hip) against the float64 oracle of tests/vm_oracle.py on every output, texel and
line node; its bit ties to the tri-plane sampler and to the float32 line restatement; the op's autograd against a float64
torch restatement; and VMTriPlaneVoxGO fused against unfused, through the training step, a checkpoint, scale_volume_grid and
render_viewpoints.

Error bounds (U = 2^-24; A = the magnitude the oracle returns), derived, not tuned:
  forward   |got - ref| <= 12 U A.  The corner weight product and its two weights account for 3 U, the four fmas for 4 U,
            the line (two weights, two fmas: the first is exact up to its product) for 3 U and the product p * l for 1 U:
            11 U, rounded up to 12 for the second-order terms.
  backward  |got - ref| <= (n + 12) U A per texel and per line node with n contributions: at most 9 U per term (the other
            factor's value as above, the products l * g and k * (l g), or p * g and w * (p g)) plus n - 1 additions, each
            rounding a partial sum of at most A, in any order of the atomics and of a lane's own run sums; rounded up.
No element is excluded from either check.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import triplane_oracle as TO
import vm_oracle as VO

pytestmark = pytest.mark.gpu

SIZES = {'xy': (5, 7), 'yz': (6, 4), 'zx': (3, 9)}
LINES = {'xy': 6, 'yz': 1, 'zx': 9}
MS = (0, 1, 63, 64, 65, 1000)
MN, MX = np.array([-1.0, -0.8, -0.6], np.float32), np.array([0.9, 1.1, 0.7], np.float32)
MODES = (1, 2)                              # the modes dvgo_vm_bwd ships (profiles/vm/README.md)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def lay_out(p, layout):
    """numpy [1,C,H,W] -> a device tensor of that shape: channel-first ('cf'), channels-last ('cl'), or a channels-last
    view that starts one float off a 16-byte boundary ('off')."""
    t = cu(p)
    if layout == 'cf':
        return t
    if layout == 'cl':
        return t.contiguous(memory_format=torch.channels_last)
    _, C, H, W = t.shape
    buf = torch.zeros(t.numel() + 1, device='cuda')
    assert buf.data_ptr() % 16 == 0
    view = buf[1:].as_strided((1, C, H, W), (H * W * C, 1, W * C, C))
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


def points(M, rng):
    """Random points up to 30 % of the box outside it; in front of them the eight box corners (both faces of every axis:
    exact lattice nodes, and on the upper face f + 1 is out of range), the lattice nodes of every plane and line, and
    points 0.8 box extents outside on each side: more than one cell of every axis here (the coarsest has 3 nodes, a
    cell of 0.5 extents), so that all corners are out."""
    xyz = (MN + (MX - MN) * (rng.random((M, 3)) * 1.6 - 0.3)).astype(np.float32)
    special = [[(MN, MX)[(i >> a) & 1][a] for a in range(3)] for i in range(8)]
    for key, (H, W) in SIZES.items():
        ah, aw = TO.AXES[key]
        al, N = VO.LINE_AXIS[key], LINES[key]
        for i in range(4):
            p = (MN + (MX - MN) * rng.random(3)).astype(np.float32)
            p[ah] = MN[ah] + (MX[ah] - MN[ah]) * np.float32((i % H) / max(H - 1, 1))
            p[aw] = MN[aw] + (MX[aw] - MN[aw]) * np.float32((i % W) / max(W - 1, 1))
            p[al] = MN[al] + (MX[al] - MN[al]) * np.float32((i % N) / max(N - 1, 1))
            special.append(p)
    for side in (-0.8, 1.8):
        special.append(MN + (MX - MN) * np.float32(side))
        for a in range(3):
            p = (MN + (MX - MN) * np.float32(0.4)).astype(np.float32)
            p[a] = MN[a] + (MX[a] - MN[a]) * np.float32(side)
            special.append(p)
    special = np.array(special, np.float32)[:M]
    xyz[:len(special)] = special
    return xyz


@functools.lru_cache(maxsize=None)
def case(R):
    """Inputs and oracle results for component count R, shared by the layouts: planes, lines and, per M, (xyz, forward
    value and A, grad_out, backward reference)."""
    rng = np.random.default_rng(100 + R)
    planes = {k: rng.standard_normal((1, R, *hw)).astype(np.float32) for k, hw in SIZES.items()}
    lines = {k: rng.standard_normal((1, R, n, 1)).astype(np.float32) for k, n in LINES.items()}
    per_m = {}
    for M in MS:
        xyz = points(M, rng)
        val, A = VO.forward(planes, lines, xyz, MN, MX)
        gout = rng.standard_normal((M, 3 * R)).astype(np.float32)
        per_m[M] = (xyz, val, A, gout, VO.backward(planes, lines, xyz, MN, MX, gout))
    return planes, lines, per_m


def test_points_cover_the_edge_cases():
    xyz = case(4)[2][1000][0]
    for key, (H, W) in SIZES.items():
        ih, iw, w, ok = TO.corners(key, H, W, xyz, MN, MX)
        assert ((w == 1).any(0)).sum() >= 8                                   # lattice nodes exactly
        assert (ok[0] & ~ok[2]).any() and (ok[0] & ~ok[1]).any()              # upper faces: h0 + 1 / w0 + 1 out of range
        assert (~ok.any(0)).sum() >= 2                                        # all four corners out
        idx, wl, okl = VO.nodes(key, LINES[key], xyz, MN, MX)
        assert (okl[0] & ~okl[1]).any() and ((wl == 1).any(0)).sum() >= 8
        if LINES[key] > 1:
            assert (~okl.any(0)).any() and (~okl[0] & okl[1]).any()           # both nodes out; only the lower one out
    val = case(4)[2][1000][1]
    assert (val[[20, 24]] == 0).all() and (val[:20] != 0).any()               # outside on every axis: an exact 0


@pytest.mark.parametrize('layout', ['cf', 'cl', 'off'])
@pytest.mark.parametrize('R', [1, 3, 4, 8])
def test_sampler_against_oracle(R, layout):
    """R = 1 and 3 take the scalar and (cf) sample-fastest branches, 4 and 8 in 'cl' the vector ones; 'off' is channels-last
    but misaligned: scalar loads, component-fastest scatter."""
    from directvoxgo_amd.ops import vm_bwd, vm_fwd
    planes, lines, per_m = case(R)
    dp = {k: lay_out(p, layout) for k, p in planes.items()}
    dl = {k: lay_out(p, layout) for k, p in lines.items()}
    mn, mx = cu(MN), cu(MX)
    worst_f = worst_b = 0.0
    for M in MS:
        xyz, val, A, gout, (rp, rl) = per_m[M]
        dx = cu(xyz).reshape(M, 3)
        got_t = vm_fwd(dp, dl, dx, mn, mx)
        got = got_t.cpu().numpy().astype(np.float64)
        assert got.shape == val.shape == (M, 3 * R)
        err, bound = np.abs(got - val), 12 * VO.U * A
        if M:
            worst_f = max(worst_f, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (M, float((err - bound).max()))
        assert torch.equal(got_t, vm_fwd(dp, dl, dx, mn, mx))                 # bitwise repeatable
        for mode in MODES:
            for run in (1, 4, 7):
                gp = {k: lay_out(np.zeros_like(p), layout) for k, p in planes.items()}
                gl = {k: lay_out(np.zeros_like(p), layout) for k, p in lines.items()}
                vm_bwd(cu(gout).reshape(M, 3 * R), dp, dl, gp, gl, dx, mn, mx, run=run, mode=mode)
                for k in VO.KEYS:
                    for name, dev, (g, Ag, n) in (('plane', gp[k][0], rp[k]), ('line', gl[k][0, :, :, 0], rl[k])):
                        gg = dev.cpu().numpy().astype(np.float64)
                        err, bound = np.abs(gg - g), (n[None] + 12) * VO.U * Ag
                        if M:
                            worst_b = max(worst_b, float((err / np.maximum(bound, 1e-300)).max()))
                        assert (err <= bound).all(), (M, mode, run, k, name, float((err - bound).max()))
                        assert (gg[:, n == 0] == 0).all(), (M, mode, run, k, name)
    print(f'R={R} {layout}: worst forward err / bound {worst_f:.3f}, worst backward err / bound {worst_b:.3f}')


def test_sampler_against_oracle_past_the_grid_cap():
    """Mode 2 launches at most 1024 workgroups, each walking a share of the lanes and adding its table once: 12 000 samples
    of R = 8 at run 1 are 288 000 lanes, 1125 workgroups' worth, the smallest round size past the cap (a share is then two
    workgroup sizes); run 4 stays below it.  Same bounds as above, both modes."""
    from directvoxgo_amd.ops import vm_bwd
    planes, lines, _ = case(8)
    rng = np.random.default_rng(77)
    M, R = 12000, 8
    xyz = points(M, rng)
    gout = rng.standard_normal((M, 3 * R)).astype(np.float32)
    rp, rl = VO.backward(planes, lines, xyz, MN, MX, gout)
    dp = {k: lay_out(p, 'cl') for k, p in planes.items()}
    dl = {k: lay_out(p, 'cl') for k, p in lines.items()}
    for mode in MODES:
        for run in (1, 4):
            gp = {k: torch.zeros_like(p) for k, p in dp.items()}
            gl = {k: torch.zeros_like(p) for k, p in dl.items()}
            vm_bwd(cu(gout), dp, dl, gp, gl, cu(xyz), cu(MN), cu(MX), run=run, mode=mode)
            for k in VO.KEYS:
                for name, dev, (g, Ag, n) in (('plane', gp[k][0], rp[k]), ('line', gl[k][0, :, :, 0], rl[k])):
                    err = np.abs(dev.cpu().numpy().astype(np.float64) - g)
                    bound = (n[None] + 12) * VO.U * Ag
                    assert (err <= bound).all(), (mode, run, k, name, float((err - bound).max()))


# ---------------------------------------------------------------------------------------------- bit ties
@pytest.mark.parametrize('layout', ['cf', 'cl'])
def test_unit_lines_give_the_triplane_samplers_bits(layout):
    """Every line of length 1 holding 1.0: l = fmaf(1, 1, 0) = 1 at every position, p * 1 = p: dvgo_triplane_fwd's 'concat'
    output, bit for bit."""
    from directvoxgo_amd.ops import triplane_fwd, vm_fwd
    planes, _, per_m = case(4)
    xyz = cu(per_m[1000][0])
    dp = {k: lay_out(p, layout) for k, p in planes.items()}
    ones = {k: lay_out(np.ones((1, 4, 1, 1), np.float32), layout) for k in VO.KEYS}
    got = vm_fwd(dp, ones, xyz, cu(MN), cu(MX))
    assert torch.equal(got, triplane_fwd(dp, xyz, cu(MN), cu(MX), 'concat')) and float(got.abs().sum()) > 0


@pytest.mark.parametrize('layout', ['cf', 'cl'])
def test_unit_planes_give_the_line_restatement(layout):
    """Every plane 1 x 1 holding 1.0: p = fmaf(1, 1 * 1, 0) = 1 at every position, 1 * l = l: the float32 restatement of
    the line sample (vm_oracle.line32: correctly rounded fmas in the stated order), bit for bit."""
    from directvoxgo_amd.ops import vm_fwd
    _, lines, per_m = case(4)
    xyz = per_m[1000][0]
    ones = {k: lay_out(np.ones((1, 4, 1, 1), np.float32), layout) for k in VO.KEYS}
    dl = {k: lay_out(p, layout) for k, p in lines.items()}
    got = vm_fwd(ones, dl, cu(xyz), cu(MN), cu(MX)).cpu().numpy()
    ref = np.concatenate([VO.line32(k, lines[k], xyz, MN, MX) for k in VO.KEYS], 1)
    assert got.dtype == ref.dtype == np.float32 and np.array_equal(got, ref) and np.abs(ref).sum() > 0


# ---------------------------------------------------------------------------------------------- other sampler and op checks
def test_bwd_accumulates_into_the_callers_buffers():
    """Two calls give twice one call, to 2 U relative.  Float atomics sum in any order, so the inputs are chosen such that
    no order can matter: planes 5 x 5 and lines 5 over [-1, 1]^3 put the lattice at multiples of 0.5, where every float32
    coordinate operation is exact, and the five diagonal nodes (i, i, i) give every texel and line node exactly one
    contribution of weight 1 beside exact zeros.  One call then leaves fl(k * fl(l * g)) in a cell, the second adds the
    same number to it: exactly twice.  A second, random case holds two calls to the oracle's bound with 2 n terms."""
    from directvoxgo_amd.ops import vm_bwd
    rng = np.random.default_rng(8)
    R = 4
    mn, mx = np.float32([-1, -1, -1]), np.float32([1, 1, 1])
    planes = {k: rng.standard_normal((1, R, 5, 5)).astype(np.float32) for k in VO.KEYS}
    lines = {k: rng.standard_normal((1, R, 5, 1)).astype(np.float32) for k in VO.KEYS}
    xyz = np.float32([[-1 + 0.5 * i] * 3 for i in range(5)])
    gout = rng.standard_normal((5, 3 * R)).astype(np.float32)
    dp = {k: lay_out(p, 'cl') for k, p in planes.items()}
    dl = {k: lay_out(p, 'cl') for k, p in lines.items()}
    for mode in MODES:
        once = [torch.zeros_like(t) for t in list(dp.values()) + list(dl.values())]
        twice = [torch.zeros_like(t) for t in once]
        vm_bwd(cu(gout), dp, dl, once[:3], once[3:], cu(xyz), cu(mn), cu(mx), mode=mode)
        for _ in range(2):
            vm_bwd(cu(gout), dp, dl, twice[:3], twice[3:], cu(xyz), cu(mn), cu(mx), mode=mode)
        for a, b in zip(once, twice):
            assert float(a.abs().sum()) > 0
            assert bool(((b - 2 * a).abs() <= 2 * VO.U * (2 * a).abs()).all())
    planes, lines, per_m = case(4)
    xyz, _, _, gout, (rp, rl) = per_m[1000]
    dp = {k: lay_out(p, 'cl') for k, p in planes.items()}
    dl = {k: lay_out(p, 'cl') for k, p in lines.items()}
    gp = [torch.zeros_like(dp[k]) for k in VO.KEYS]
    gl = [torch.zeros_like(dl[k]) for k in VO.KEYS]
    for _ in range(2):
        vm_bwd(cu(gout), dp, dl, gp, gl, cu(xyz), cu(MN), cu(MX))
    for i, k in enumerate(VO.KEYS):
        for dev, (g, Ag, n) in ((gp[i][0], rp[k]), (gl[i][0, :, :, 0], rl[k])):
            err = np.abs(dev.cpu().numpy().astype(np.float64) - 2 * g)
            assert (err <= (2 * n[None] + 12) * VO.U * 2 * Ag).all()


def _dyadic_case(rng, M=300, R=4):
    """Box [-1, 1]^3 and points on multiples of 2^-10 in [-1.25, 1.25]: every float32 coordinate operation of the kernel
    (p - min, / 2, * 2 - 1, + 1, / 2, * (size - 1), floor and the weights) is then exact, so a float64 evaluation sees
    the same cells and weights and the comparison is about the sampler's own arithmetic."""
    mn, mx = np.float32([-1, -1, -1]), np.float32([1, 1, 1])
    xyz = (rng.integers(-1280, 1281, (M, 3)) / 1024.0).astype(np.float32)
    planes = {k: (0.5 * rng.standard_normal((1, R, *hw))).astype(np.float32) for k, hw in SIZES.items()}
    lines = {k: (0.5 * rng.standard_normal((1, R, n, 1))).astype(np.float32) for k, n in LINES.items()}
    gout = rng.standard_normal((M, 3 * R)).astype(np.float32)
    return mn, mx, xyz, planes, lines, gout


@pytest.mark.parametrize('wants', ['both', 'planes', 'lines'])
@pytest.mark.parametrize('layout', ['cf', 'cl'])
def test_op_autograd_against_the_float64_restatement(layout, wants):
    """ops.vm_sample against six float64 F.grid_sample, product and cat on the CPU, at section 6's tolerances for this kind
    of comparison: values rtol 1e-5 / atol 1e-6, gradients rtol 1e-4 / atol 1e-6.  Channel-first inputs are handed to the
    kernels as channels-last copies (the samples outnumber the texels).  With only the planes or only the lines requiring a
    gradient the other three get none."""
    from directvoxgo_amd.ops import vm_sample
    mn, mx, xyz, planes, lines, gout = _dyadic_case(np.random.default_rng(21))
    t64 = lambda d, rg: {k: torch.from_numpy(v).double().requires_grad_(rg) for k, v in d.items()}          # noqa: E731
    rp, rl = t64(planes, True), t64(lines, True)
    ref = VO.torch_restatement(rp, rl, torch.from_numpy(xyz).double(), torch.from_numpy(mn).double(), torch.from_numpy(mx).double())
    ref.backward(torch.from_numpy(gout).double())
    dp = {k: lay_out(p, layout).requires_grad_(wants in ('both', 'planes')) for k, p in planes.items()}
    dl = {k: lay_out(p, layout).requires_grad_(wants in ('both', 'lines')) for k, p in lines.items()}
    out = vm_sample(dp, dl if layout == 'cf' else [dl[k] for k in VO.KEYS], cu(xyz), cu(mn), cu(mx))
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), rtol=1e-5, atol=1e-6)
    out.backward(cu(gout))
    for dev, refs, on in ((dp, rp, wants != 'lines'), (dl, rl, wants != 'planes')):
        for k in VO.KEYS:
            if not on:
                assert dev[k].grad is None
                continue
            assert dev[k].grad.shape == dev[k].shape
            np.testing.assert_allclose(dev[k].grad.cpu().numpy(), refs[k].grad.numpy(), rtol=1e-4, atol=1e-6)
    shaped = vm_sample(dp, dl, cu(xyz).reshape(15, 20, 3), cu(mn), cu(mx))
    assert shaped.shape == (15, 20, out.shape[1]) and torch.equal(shaped.reshape(300, -1), out)


# ---------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope='module')
def scene():
    from directvoxgo_amd.scenes import synthetic_scene
    return synthetic_scene(world=32, n_rays=2048, seed=6, device='cuda')


def _scene_model(sc, fused=True, seed=1, **kw):
    from directvoxgo_amd.vm import VMTriPlaneVoxGO
    torch.manual_seed(seed)
    m = VMTriPlaneVoxGO(sc['xyz_min'], sc['xyz_max'], **{**dict(
        num_voxels=sc['world'] ** 3, num_voxels_base=sc['world'] ** 3, alpha_init=1e-2, fast_color_thres=1e-4, n_comp=8,
        rgbnet_dim=6, rgbnet_width=64, fused=fused), **kw})
    for p in m.rgbnet.parameters():
        torch.nn.init.normal_(p, std=0.1)
    m = m.cuda()
    with torch.no_grad():
        m.density.copy_(sc['density']); m.mask_cache.mask.copy_(sc['mask'])
    return m


def test_fused_equals_unfused(scene):
    """Both paths call the same sampler on bit-equal positions: ray_id and the features are equal, and with the same colour
    head (torch's) behind them so are weights, raw_rgb, rgb_marched and depth."""
    from directvoxgo_amd.fused import fused_march
    from directvoxgo_amd.ops import Alphas2Weights
    sc = scene
    ro, rd, vd = sc['rays_o'], sc['rays_d'], sc['viewdirs']
    rk = dict(near=sc['near'], far=sc['far'], bg=1, stepsize=0.5, render_depth=True)
    outs, featv = {}, {}
    for fused in (True, False):
        m = _scene_model(sc, fused=fused)
        m.fused_shade = False
        with torch.no_grad():
            outs[fused] = m(ro, rd, vd, **rk)
            if fused:
                cfg = m._march_cfg(rk['near'], rk['far'], rk['stepsize'])
                pts = fused_march(m.density, m.density.detach()[:, :0], ro, rd, cfg, positions=True)[3]
            else:
                pts, rid, sid = m.sample_ray(rays_o=ro, rays_d=rd, **rk)
                keep = m.mask_cache(pts)
                pts, rid = pts[keep], rid[keep]
                alpha = m.activate_density(m.grid_sampler(pts, m.density), rk['stepsize'] * m.voxel_size_ratio)
                keep = alpha > m.fast_color_thres
                pts, rid, alpha = pts[keep], rid[keep], alpha[keep]
                w, _ = Alphas2Weights.apply(alpha, rid, ro.shape[0])
                pts = pts[w > m.fast_color_thres]
            featv[fused] = m.sample_planes(pts)
    a, b = outs[True], outs[False]
    assert a['ray_id'].shape[0] > 1000 and featv[True].shape == (a['ray_id'].shape[0], 6)
    assert np.array_equal(a['ray_id'].cpu().numpy(), b['ray_id'].cpu().numpy())
    assert torch.equal(featv[True], featv[False]) and float(featv[True].abs().sum()) > 0
    for k in ('weights', 'raw_rgb', 'rgb_marched', 'depth'):
        assert torch.equal(a[k], b[k]), k


def test_external_planes_and_lines(scene):
    """render(feats): planes from the caller, lines from the caller where given and the model's own otherwise; gradients
    reach the caller's tensors."""
    sc = scene
    m = _scene_model(sc)
    rk = dict(near=sc['near'], far=sc['far'], bg=1, stepsize=0.5)
    args = (sc['rays_o'], sc['rays_d'], sc['viewdirs'])
    feats = {k: (p.detach() * 2).requires_grad_() for k, p in m.planes.items()}
    own = m(*args, **rk)['rgb_marched']
    ext = m.render(feats, *args, **rk)['rgb_marched']
    assert not torch.equal(own, ext)
    ext.sum().backward()
    assert all(float(f.grad.abs().sum()) > 0 for f in feats.values()) and m.planes['xy'].grad is None
    assert float(m.lines['xy'].grad.abs().sum()) > 0
    feats2 = {**{k: p.detach() for k, p in m.planes.items()}, 'yz_line': (m.lines['yz'].detach() * 0).requires_grad_()}
    pts = sc['rays_o'][:64] * 0.1
    f2 = m.sample_planes(pts, feats2)
    full = m.sample_planes(pts)
    lines0 = {k: (ln.detach() * (0 if k == 'yz' else 1)) for k, ln in m.lines.items()}
    from directvoxgo_amd.ops import vm_sample
    assert torch.equal(f2, vm_sample(m.planes, lines0, pts, m.xyz_min, m.xyz_max) @ m.basis) and not torch.equal(f2, full)


def test_train_step_checkpoint_and_scale_volume_grid(scene, tmp_path):
    """Three TrainStep steps with VM_FINE_TRAIN lower the loss and move density, planes, lines, basis and MLP; a checkpoint
    loaded into a fresh model gives equal state_dicts and an equal render; scale_volume_grid resizes planes and lines that
    follow world_size and leaves fixed-size ones alone."""
    from directvoxgo_amd.checkpoint import load_model, save_checkpoint
    from directvoxgo_amd.train import TrainStep
    from directvoxgo_amd.vm import VM_FINE_TRAIN, VMTriPlaneVoxGO
    sc = scene
    rk = dict(near=sc['near'], far=sc['far'], bg=1, stepsize=0.5)
    m = _scene_model(sc)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    step = TrainStep(m, dict(VM_FINE_TRAIN), rk)
    assert not step.can_capture()
    args = (sc['rays_o'], sc['rays_d'], sc['viewdirs'], sc['target'])
    losses = [float(step(*args, global_step=s)) for s in (1, 2, 3)]
    print('losses', losses)
    assert losses[2] < losses[0]
    after = m.state_dict()
    for k in ('density', 'planes.xy', 'planes.yz', 'planes.zx', 'lines.xy', 'lines.yz', 'lines.zx', 'basis', 'rgbnet.0.weight',
              'rgbnet.3.bias'):
        assert not torch.equal(before[k], after[k]), k
    path = str(tmp_path / 'vm.tar')
    save_checkpoint(path, m, step.optimizer, 3)
    m2 = load_model(VMTriPlaneVoxGO, path).cuda()
    assert m2.n_comp == 8 and m2.line_size is None
    assert set(m2.state_dict()) == set(after) and all(torch.equal(v, m2.state_dict()[k]) for k, v in after.items())
    with torch.no_grad():
        ra, rb = m(*args[:3], render_depth=True, **rk), m2(*args[:3], render_depth=True, **rk)
    assert all(torch.equal(ra[k], rb[k]) for k in ('rgb_marched', 'depth', 'weights', 'ray_id'))

    old = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m.scale_volume_grid(40 ** 3)
    ws = tuple(int(v) for v in m.world_size)
    assert min(ws) > 32 and tuple(m.density.shape[2:]) == ws
    for k in VO.KEYS:
        hw = (ws[TO.AXES[k][0]], ws[TO.AXES[k][1]])
        p, ln = m.planes[k], m.lines[k]
        ref = F.interpolate(old['planes.' + k].contiguous(), size=hw, mode='bilinear', align_corners=True)
        assert tuple(p.shape) == (1, 8, *hw) and p.stride(1) == 1 and torch.equal(p.detach(), ref)
        n = ws[VO.LINE_AXIS[k]]
        ref = F.interpolate(old['lines.' + k].contiguous(), size=(n, 1), mode='bilinear', align_corners=True)
        assert tuple(ln.shape) == (1, 8, n, 1) and ln.stride(1) == 1 and torch.equal(ln.detach(), ref)
    assert torch.isfinite(m(*args[:3], **rk)['rgb_marched']).all()
    fixed = _scene_model(sc, plane_size=(20, 24), line_size=11)
    held = {k: v.detach().clone() for k, v in fixed.state_dict().items() if k.startswith(('planes', 'lines'))}
    fixed.scale_volume_grid(40 ** 3)
    assert tuple(fixed.density.shape[2:]) == ws and all(torch.equal(v, fixed.state_dict()[k]) for k, v in held.items())
    assert all(tuple(p.shape) == (1, 8, 20, 24) for p in fixed.planes.values())
    assert all(tuple(p.shape) == (1, 8, 11, 1) for p in fixed.lines.values())


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
