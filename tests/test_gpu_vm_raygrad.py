"""GPU: the vector-matrix samplers' position gradient (csrc/vm_xyz.hip), from the kernel to pose refinement.

  * both entries against tests/vm_raygrad_oracle.py (bound gamma(R + 12 + SLACK) mag + tiny, exact zeros where nothing
    contributes) on the cases tests/test_vm_raygrad_host.py holds the float32 restatement to: R in (1, 4, 5, 16), contiguous
    and channels-last planes and lines (both VEC paths), non-square planes, H = 1, N = 1, M in (1, 63, 64, 65, 1000),
    lattice nodes, faces, up to and beyond one cell outside, NaN rows; the two layouts give the same bits;
  * ops.vm_sample / ops.vm_density: position_grad=True gives the kernel's rows beside the unchanged plane and line
    gradients, the default call launches what it launched and leaves xyz.grad None;
  * VMTriPlaneVoxGO / TensoRFVoxGO(raygrad=True): rays that require grad give the op-by-op forward's bits in every key,
    caller-supplied feats included; the ray gradients against tests/vm_render_oracle.py, the render restated on the float32
    run's cells in float64 and float32 (device error <= 4 x the float32 restatement's own), with the share that passes
    through the VM tensors above 100 x that tolerance on at least half of the rays that reach a kept sample;
  * refine_poses on a perturbed 6-view 24 x 24 capture (tests/hash_render_oracle.capture, the capture of
    tests/test_gpu_hash_raygrad.py at half its perturbation, fixed by tools/vm_raygrad_descent_cpu.py): every view recovers
    with the model frozen, and poses and model are stepped together.
"""
import math

import numpy as np
import pytest
import torch

import hash_render_oracle as RO
import vm_raygrad_oracle as VR
import vm_render_oracle as VRO

pytestmark = pytest.mark.gpu

f32 = np.float32
WORST = {}


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print(f'\n{k}: {WORST[k]}', end='')
    print()


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = host(a) if isinstance(a, torch.Tensor) else a, host(b) if isinstance(b, torch.Tensor) else b
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _device(planes, lines, channels_last):
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    return ({k: cu(v).contiguous(memory_format=fmt) for k, v in planes.items()},
            {k: cu(v).contiguous(memory_format=fmt) for k, v in lines.items()})


# ------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize('R', VR.RS)
@pytest.mark.parametrize('shape', sorted(VR.SHAPES))
def test_kernels_inside_the_oracle_bound(shape, R):
    from directvoxgo_amd import ops
    rng = np.random.default_rng(500 + R)                     # the cases of tests/test_vm_raygrad_host.py, by construction
    planes, lines = VR.tensors(shape, R, rng)
    mn, mx = cu(VR.MN), cu(VR.MX)
    for M in VR.MS:
        xyz_np = VR.points(M, rng)
        g_feat, g_dens = rng.standard_normal((M, 3 * R)).astype(f32), rng.standard_normal(M).astype(f32)
        g_dens[::7] = 0
        xyz = cu(xyz_np)
        for what, fn, gout in (('vm_bwd_xyz', ops.vm_bwd_xyz, g_feat), ('vm_density_bwd_xyz', ops.vm_density_bwd_xyz, g_dens)):
            got = {}
            for cl in (False, True):
                P, Ln = _device(planes, lines, cl)
                got[cl] = host(fn(cu(gout), P, Ln, xyz, mn, mx))
                assert same_bits(got[cl], fn(cu(gout), P, Ln, xyz, mn, mx))          # one fixed summation order
            assert same_bits(got[False], got[True])                                  # VEC and layout do not change the bits
            S = VR.sums(planes, lines, gout, xyz_np, VR.MN, VR.MX)
            r = VR.check(S, got[True], what=f'{what} {shape} R={R} M={M}')
            key = f'worst err / bound  {what} {shape} R={R}'
            WORST[key] = max(WORST.get(key, 0.0), r)
            if M == 1000:
                inside = VR.in_box(xyz_np)
                if gout.ndim == 1:
                    assert np.all(got[True][gout == 0] == 0)
                    inside &= gout != 0
                assert (np.abs(S.ref[inside]) > 100 * S.bound()[inside]).mean() >= 0.5     # zeros could not pass
                nan = np.isnan(xyz_np).any(1)
                assert nan.sum() == 2 and np.all(got[True][nan] == 0)
                outside = ~inside & ~nan
                assert (np.abs(got[True][outside]).max(1) > 0).sum() >= 50           # less than one cell outside: not zero


# ------------------------------------------------------------------------------------------ the ops
@pytest.mark.parametrize('density', [False, True])
def test_ops_with_position_gradient(density):
    from directvoxgo_amd import _lib, ops
    rng = np.random.default_rng(71)
    R, M = 4, 300
    planes, lines = VR.tensors('base', R, rng)
    xyz_np = VR.points(M, rng)
    xyz_np = xyz_np[~np.isnan(xyz_np).any(1)]
    M = len(xyz_np)
    gout_np = rng.standard_normal(M if density else (M, 3 * R)).astype(f32)
    mn, mx = cu(VR.MN), cu(VR.MX)
    op = ops.vm_density if density else ops.vm_sample
    low = ops.vm_density_bwd_xyz if density else ops.vm_bwd_xyz
    entry = 'dvgo_vm_density_bwd_xyz' if density else 'dvgo_vm_bwd_xyz'
    r, calls = {}, {}
    real = _lib.call
    for pg in (False, True):
        P, Ln = _device(planes, lines, True)
        for t in list(P.values()) + list(Ln.values()):
            t.requires_grad_()
        x = cu(xyz_np).requires_grad_()
        seen = []
        _lib.call = lambda name, *a: (seen.append(name), real(name, *a))[1]
        ops.L.call = _lib.call
        try:
            out = op(P, Ln, x, mn, mx, position_grad=pg) if pg else op(P, Ln, x, mn, mx)
            out.backward(cu(gout_np))
        finally:
            _lib.call = real
            ops.L.call = real
        calls[pg] = seen
        r[pg] = (out.detach(), [t.grad for t in list(P.values()) + list(Ln.values())], x.grad)
    assert same_bits(r[False][0], r[True][0])                                     # the same forward launch, the same bits
    assert r[False][2] is None and r[True][2] is not None and r[True][2].shape == (M, 3)
    assert entry not in calls[False] and len(calls[False]) == 2                   # forward and scatter, as before
    assert calls[True] == [calls[False][0], entry, calls[False][1]]               # the position kernel ahead of the scatter
    S = VR.sums(planes, lines, gout_np, xyz_np, VR.MN, VR.MX)
    WORST[f'worst err / bound  ops xyz.grad density={density}'] = VR.check(S, host(r[True][2]), what='xyz.grad')
    P, Ln = _device(planes, lines, True)
    assert same_bits(r[True][2], low(cu(gout_np), P, Ln, cu(xyz_np), mn, mx))      # the kernel's rows
    for a, b in zip(r[False][1], r[True][1]):                                     # both gradients in one backward: the scatter
        assert a is not None and torch.allclose(a, b, rtol=1e-4, atol=1e-5)       # is the separate call's (float atomics)
    # frozen planes and lines: the position kernel alone
    P, Ln = _device(planes, lines, True)
    x = cu(xyz_np.reshape(-1, 1, 3)).requires_grad_()
    seen = []
    _lib.call = lambda name, *a: (seen.append(name), real(name, *a))[1]
    ops.L.call = _lib.call
    try:
        op(P, Ln, x, mn, mx, position_grad=True).backward(cu(gout_np.reshape(M, 1, -1) if not density else gout_np.reshape(M, 1)))
    finally:
        _lib.call = real
        ops.L.call = real
    assert seen[1:] == [entry] and same_bits(x.grad.reshape(M, 3), r[True][2])


# ------------------------------------------------------------------------------------------ the models
RK = dict(near=2.0, far=6.0, stepsize=0.5, bg=1, render_depth=True)
WORLD = 32


make_model = VRO.make_model


@pytest.fixture(scope='module')
def rays():
    from directvoxgo_amd import scenes
    sc = scenes.synthetic_scene(world=WORLD, n_rays=256)
    assert RK['near'] == sc['near'] and RK['far'] == sc['far'] and RK['stepsize'] == sc['stepsize']
    assert abs(float(sc['xyz_max'][0]) - RO.HALF) < 1e-6
    return sc['rays_o'].cuda(), sc['rays_d'].cuda(), sc['viewdirs'].cuda()


def _dict_bits_equal(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert same_bits(a[k], b[k]), k


@pytest.mark.parametrize('which', ['vm', 'tensorf'])
def test_forward_bits_and_ray_gradients(which, rays):
    o, d, v = rays
    m = make_model(which, WORLD, seed=3).cuda()
    assert m.raygrad and m.fused
    # the op-by-op forward on the same detached rays
    with torch.no_grad():
        pts, ray_id, step_id = m.sample_ray(o, d, **RK)
        keep = m.mask_cache(pts)
        want = m._forward_unfused(len(o), v, RK['stepsize'], RK['bg'], True, pts[keep], ray_id[keep], step_id[keep])
    # rays that reach a kept sample, of synthetic_scene(world=32, n_rays=256)'s 256: 96 for 'vm' (the blob subtends about a
    # third of the cameras' field of view), all 256 for 'tensorf' (the negative constant leaves alpha above 1e-4 everywhere)
    n_reached = int(torch.unique(want['ray_id']).numel())
    WORST[f'{which}: rays that reach a kept sample (of 256)'] = n_reached
    assert n_reached == {'vm': 96, 'tensorf': 256}[which] and n_reached >= 64
    og, dg = o.clone().requires_grad_(), d.clone().requires_grad_()
    res = m(og, dg, v, **RK)
    assert res['rgb_marched'].requires_grad
    _dict_bits_equal(want, res)
    if which == 'tensorf':                                   # whatever fused_march says
        m.fused_march = True
        try:
            _dict_bits_equal(want, m(o.clone().requires_grad_(), d, v, **RK))
        finally:
            m.fused_march = False
    with torch.no_grad():                                    # rays that do not ask: exactly the default model
        m.raygrad = False
        try:
            default = m(o, d, v, **RK)
        finally:
            m.raygrad = True
        _dict_bits_equal(default, m(og, dg, v, **RK))
    # caller-supplied tensors keep working and take their gradient
    feats = {**{k: p.detach() for k, p in m.planes.items()}, 'xy': (m.planes['xy'].detach() * 0.5).requires_grad_(),
             'zx_line': m.lines['zx'].detach().clone().requires_grad_()}
    if which == 'tensorf':
        feats['yz_density'] = (m.density_planes['yz'].detach() * 0.9).requires_grad_()
    with torch.no_grad():
        want_f = m._forward_unfused(len(o), v, RK['stepsize'], RK['bg'], True, pts[keep], ray_id[keep], step_id[keep], feats=feats)
    o2 = o.clone().requires_grad_()
    res_f = m.render(feats, o2, d, v, **RK)
    _dict_bits_equal(want_f, res_f)
    assert not same_bits(res_f['rgb_marched'], res['rgb_marched'])
    res_f['rgb_marched'].square().sum().backward()
    assert all(float(feats[k].grad.abs().sum()) > 0 for k in feats if feats[k].requires_grad)
    assert m.planes['xy'].grad is None and bool(torch.isfinite(o2.grad).all()) and float(o2.grad.abs().sum()) > 0
    # the ray gradients: finite, non-zero on the rays that reach a kept sample, exactly zero on the others, and the VM
    # tensors carry a share of them
    m.zero_grad(set_to_none=True)
    tgt = torch.linspace(0.1, 0.9, 3, device='cuda')
    (res['rgb_marched'] - tgt).square().sum().backward()
    reached = torch.zeros(len(o), dtype=torch.bool, device='cuda')
    reached[want['ray_id'].long()] = True
    for g in (og.grad, dg.grad):
        assert bool(torch.isfinite(g).all()) and bool((g[~reached] == 0).all())
        assert int((g[reached].abs().sum(1) > 0).sum()) >= 0.9 * n_reached
    og2, dg2 = o.clone().requires_grad_(), d.clone().requires_grad_()
    saved = {k: p.detach().clone() for k, p in m.lines.items()}
    with torch.no_grad():
        for p in m.lines.values():                            # constant lines: the features lose their dn share
            p.copy_(p.mean(2, keepdim=True).expand_as(p))
    (m(og2, dg2, v, **RK)['rgb_marched'] - tgt).square().sum().backward()
    with torch.no_grad():
        for k, p in m.lines.items():
            p.copy_(saved[k])
    assert not torch.allclose(og2.grad, og.grad, rtol=1e-3, atol=1e-7)


def _device_record(m, o, d):
    """What the restatement takes from the device run: the kept-sample sets, lam and the float32 cells."""
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
        alpha = m.activate_density(m._raw_density(pts), RK['stepsize'] * m.voxel_size_ratio)
        m1 = alpha > m.fast_color_thres
        w1, _ = Alphas2Weights.apply(alpha[m1].contiguous(), ray_id[m1].contiguous(), len(o))
        m2 = w1 > m.fast_color_thres
    return dict(ray_id0=ray_id.cpu(), lam=lam.cpu(), m1=m1.cpu(), act1=(w1 != 0).cpu(), m2=m2.cpu(), cells=VRO.cells_of(m, host(pts)))


def _ray_grads(m, o, d, v, rec, dtype, vm_positions=True):
    o = o.detach().cpu().to(dtype).requires_grad_()
    d = d.detach().cpu().to(dtype).requires_grad_()
    marched = VRO.restate(m, o, d, v, rec, dtype, RK, vm_positions)
    if not marched.requires_grad:                            # (TensoRFVoxGO: nothing but the VM tensors carries the gradient)
        return torch.zeros_like(o).double(), torch.zeros_like(d).double(), marched.double()
    go, gd = torch.autograd.grad(marched.square().sum(), (o, d))
    return go.double(), gd.double(), marched.detach().double()


@pytest.mark.parametrize('which', ['vm', 'tensorf'])
def test_ray_gradients_match_the_float64_restatement(which, rays):
    """The device's rays_o.grad / rays_d.grad against float64 torch.autograd of the render restated on the float32 run's
    cells (tests/vm_render_oracle.py).  e32 is the error of the same restatement in float32 against the float64 one; the
    device's may be 4 x that (the factor and the form are tests/test_gpu_hash_raygrad.py's: measured against the reference,
    not against the kernel).  The share of the gradient that passes through the VM tensors (the float64 restatement with and
    without their positions attached: the features', and in TensoRFVoxGO the density's as well, which there is all of it)
    must exceed 100 x that tolerance on at least half of the rays that reach a kept sample, so that a kernel that returned
    zeros, or dropped or mis-signed one of its three terms, could not pass.  On the CPU restatement with the oracle's sampler
    (model seed 3):
        vm       96 rays reach a kept sample (1865 samples); rays_o: max |g64| 16.3, e32 1.31e-5, median share 0.0308, above
                 100 x 4 e32 on 68 of the 96 (0.71); rays_d: max |g64| 63.2, e32 4.98e-5, median share 0.119, 67 of 96 (0.70)
        tensorf  256 rays reach a kept sample (12374 samples); rays_o: max |g64| 11.1, e32 1.15e-5, median share 0.305, above
                 on all 256; rays_d: max |g64| 38.8, e32 3.63e-5, median share 1.03, all 256"""
    o, d, v = rays
    m = make_model(which, WORLD, seed=3).cuda()
    ro, rd = o.clone().requires_grad_(), d.clone().requires_grad_()
    res = m(ro, rd, v, **RK)
    res['rgb_marched'].square().sum().backward()
    assert ro.grad is not None and rd.grad is not None
    rec = _device_record(m, o, d)
    assert same_bits(rec['ray_id0'][rec['m1']][rec['m2']], res['ray_id'])         # the record is this forward's
    o64, d64, marched64 = _ray_grads(m, o, d, v, rec, torch.float64)
    o32, d32, _ = _ray_grads(m, o, d, v, rec, torch.float32)
    on, dn, _ = _ray_grads(m, o, d, v, rec, torch.float64, vm_positions=False)    # what does not pass through the VM tensors
    assert float((marched64 - res['rgb_marched'].detach().cpu().double()).abs().max()) < 1e-4   # (the restatement is this render)
    hit = torch.zeros(len(o), dtype=torch.bool)
    hit[res['ray_id'].cpu()] = True
    assert int(hit.sum()) >= 64
    for what, g64, g32, gn, dev in (('rays_o.grad', o64, o32, on, ro.grad), ('rays_d.grad', d64, d32, dn, rd.grad)):
        e32 = float((g32 - g64).abs().max())
        err = float((dev.detach().cpu().double() - g64).abs().max())
        share = (g64 - gn).abs().amax(-1)                                         # through the VM tensors, per ray
        if (~hit).any():
            assert float(share[~hit].abs().max()) == 0
        frac = float((share[hit] > 100 * 4 * e32).float().mean())
        WORST[f'end to end {which} {what}'] = (f'max |g64| {float(g64.abs().max()):.4g}  e32 {e32:.4g}  device error {err:.4g}  (allowed '
                                               f'{4 * e32:.4g})  VM share: median {float(share[hit].median()):.4g}, above 100 x allowed on '
                                               f'{frac:.2f} of the {int(hit.sum())} rays with samples')
        print('\n', WORST[f'end to end {which} {what}'])
        assert float(g64.abs().max()) > 1e-3 and e32 > 0
        assert err <= 4 * e32, (what, err, e32)
        assert frac >= 0.5, (what, frac)                     # a kernel that returned zeros could not pass


# ------------------------------------------------------------------------------------------ pose refinement
MODEL_SEED, CAPTURE = 5, dict(n_views=6, hw=24, focal=30.0, seed=7, rot_deg=1.0, shift=0.015)
LRATE_POSE = 4e-3
RK_POSE = dict(near=2.0, far=6.0, stepsize=0.5, bg=1)


def _capture(m):
    """-> true, noisy, HW, Ks of CAPTURE and the images `m` renders from the true poses"""
    from directvoxgo_amd.pose import CameraRefiner
    true, noisy, HW, Ks = RO.capture(**CAPTURE)
    n, hw = len(true), int(HW[0, 0])
    exact = CameraRefiner(true, HW, Ks).cuda()
    view = torch.arange(n, device='cuda').repeat_interleave(hw * hw)
    p = torch.arange(hw * hw, device='cuda').repeat(n)
    with torch.no_grad():
        o, d, v = exact.rays(view, p % hw, p // hw)
        images = m(o, d, v, **RK_POSE)['rgb_marched'].reshape(n, hw, hw, 3)
    assert float(images.std()) > 0.05                         # there is something to register against
    return true, noisy, HW, Ks, images


@pytest.mark.parametrize('which', ['vm', 'tensorf'])
def test_refine_poses_recovers_a_perturbed_capture(which):
    """The capture was fixed by the float64 CPU restatement of the same descent, `python tools/vm_raygrad_descent_cpu.py --model
    vm|tensorf --rot 1.0 --shift 0.015` (world 32, model seed 5, 6 views of 24 x 24, focal 30, capture seed 7, 1 deg, shift
    0.015 of the radius, lrate 4e-3, 200 iterations on all pixels):
        vm       loss 8.159e-04 -> 1.599e-10; rotation error (deg) [1] * 6 -> [0.023, 0.006, 0.0, 0.024, 0.0, 0.014];
                 translation error [0.06] * 6 -> [0.0, 0.0006, 0.0, 0.0, 0.0, 0.0014]
        tensorf  loss 9.406e-04 -> 3.621e-08; rotation error (deg) [1] * 6 -> [0.119, 0.273, 0.0, 0.024, 0.0, 0.26];
                 translation error [0.06] * 6 -> [0.0047, 0.0168, 0.0, 0.0, 0.0, 0.0116]
    so every view ends at a third of its initial error or less.  The hash model's perturbation (2 deg, shift 0.03) was not
    taken: there the same tool leaves view 5 above its start (vm 2.52 deg and 0.1765, tensorf 2.318 deg), as the device does
    (2.532 deg, 0.1773; 2.307 deg), and at lrate 2e-3 the smaller perturbation is not recovered in 200 iterations either
    (vm view 5: 1.123 deg)."""
    from directvoxgo_amd.pose import CameraRefiner, refine_poses
    from directvoxgo_amd.tensorf import TENSORF_FINE_TRAIN
    m = make_model(which, WORLD, seed=MODEL_SEED).cuda()
    for p in m.parameters():
        p.requires_grad_(False)
    true, noisy, HW, Ks, images = _capture(m)
    ref = CameraRefiner(noisy, HW, Ks).cuda()
    rot0, tr0 = RO.pose_errors(ref.poses(), true)
    cfg = dict(TENSORF_FINE_TRAIN, weight_entropy_last=0.0, weight_rgbper=0.0)
    losses = refine_poses(m, ref, images, cfg, RK_POSE, n_iters=200, n_rand=None, lrate_pose=LRATE_POSE)
    rot1, tr1 = RO.pose_errors(ref.poses(), true)
    WORST[f'refine_poses {which}'] = (f'loss {losses[0]:.3e} -> {losses[-1]:.3e}; rotation error (deg) '
                                      f'{np.degrees(rot0.numpy()).round(3).tolist()} -> {np.degrees(rot1.numpy()).round(3).tolist()}; '
                                      f'translation error {tr0.numpy().round(4).tolist()} -> {tr1.numpy().round(4).tolist()}')
    print('\n', which, WORST[f'refine_poses {which}'])
    assert len(losses) == 200 and all(math.isfinite(x) for x in losses)
    assert losses[-1] < losses[0]
    assert bool((rot1 < rot0).all()) and bool((tr1 < tr0).all())
    assert all(q.grad is None for q in m.parameters())       # a frozen model is left alone


@pytest.mark.parametrize('which', ['vm', 'tensorf'])
def test_refine_poses_steps_poses_and_model_together(which):
    """train_model=True for 20 iterations: every trained tensor and delta receive a finite, non-zero gradient in the same
    iteration, and a frozen model's `.grad` stays untouched over 5 iterations with finite, falling losses."""
    from directvoxgo_amd.pose import CameraRefiner, refine_poses
    from directvoxgo_amd.tensorf import TENSORF_FINE_TRAIN
    m2 = make_model(which, WORLD, seed=MODEL_SEED).cuda()
    true, noisy, HW, Ks, images = _capture(m2)
    frozen = CameraRefiner(noisy, HW, Ks).cuda()
    cfg = dict(TENSORF_FINE_TRAIN, weight_entropy_last=0.0, weight_rgbper=0.0)
    first = refine_poses(m2, frozen, images, cfg, RK_POSE, n_iters=5, n_rand=None, lrate_pose=LRATE_POSE)
    assert all(math.isfinite(x) for x in first) and first[-1] < first[0]
    assert all(q.grad is None for q in m2.parameters()) and float(frozen.delta.detach().abs().sum()) > 0
    ref2 = CameraRefiner(noisy, HW, Ks).cuda()
    before = m2.planes['xy'].detach().clone()
    losses2 = refine_poses(m2, ref2, images, dict(TENSORF_FINE_TRAIN), RK_POSE, n_iters=20, n_rand=1024, lrate_pose=LRATE_POSE,
                           train_model=True, seed=1)
    assert len(losses2) == 20 and all(math.isfinite(x) for x in losses2)
    trained = list(m2.planes.values()) + list(m2.lines.values()) + [m2.basis] + list(m2.rgbnet.parameters())
    trained += [m2.density] if which == 'vm' else list(m2.density_planes.values()) + list(m2.density_lines.values())
    for q in trained + [ref2.delta]:
        assert q.grad is not None and bool(torch.isfinite(q.grad).all()) and float(q.grad.abs().sum()) > 0
    assert not torch.equal(before, m2.planes['xy'].detach()) and float(ref2.delta.detach().abs().sum()) > 0
