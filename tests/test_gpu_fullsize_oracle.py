"""GPU: the product at the sizes it exists for, against the CPU oracle (tests/render_oracle.py, pinned to the reference's
orchestration by tests/test_render_oracle_host.py), not against another HIP path.

  roofline  160^3 x 12, 8192 rays x 256 samples, every sample kept, 128-wide rgbnet_direct head (bench.py's case)
  lego      160^3 lego-like scene: mask, both filters, early stop; hit test; one training step (Adam in the brick kernel)
  config 5  256^3 x 12 inverse_y render of an 800 x 800 view (805 MB channels-last k0): three 2048-pixel slices
  config 4  DirectMPIGO 343 x 382 x 128 x 9, 4096 rays x 255 NDC samples, 64-wide head; dense TV on both grids

Per-sample features are compared bit for bit (march.hip's gather runs the dvgo_tri_setup / fmaf sequence of the
oracle's grid_sample_fwd); transmittance values to the activation's allowance (exp2/log2 against powf, common.h); the
colour head and its weight gradients against a float64 head; grid gradients to summation order, with equal sets of
touched voxels (the masked Adam branches on them).
"""
import numpy as np
import pytest
import torch

import march_oracle as MO
import render_oracle as R

pytestmark = pytest.mark.gpu


def _host_scene(m):
    """The model's grids, mask and head as the oracle reads them (k0 stays a channels-last view)."""
    mpi = getattr(m, 'mpi_depth', 0)
    head = None if m.rgbnet is None else {k: v.detach().cpu().numpy() for k, v in m.rgbnet.state_dict().items()}
    k0 = m.k0.detach().cpu().numpy()
    return R.Scene(m.xyz_min.cpu().numpy(), m.xyz_max.cpu().numpy(), m.density.detach().cpu().numpy(), k0,
                   m.mask_cache.mask.cpu().numpy(), m.fast_color_thres, act_shift=float(m.act_shift),
                   voxel_size=None if mpi else float(m.voxel_size), voxel_size_ratio=float(m.voxel_size_ratio),
                   rgbnet=head, direct=bool(mpi) or bool(getattr(m, 'rgbnet_direct', True)),
                   viewbase_pe=int(m.viewfreq.numel()) if m.rgbnet is not None else 0, mpi_depth=mpi)


def _np(t):
    return t.detach().cpu().numpy()


def _within(a, b, frac, what):
    """max |a - b| <= frac * max |b|"""
    err, scale = float(np.abs(a - b).max()), float(np.abs(b).max())
    assert scale > 0 and err <= frac * scale, (what, err, scale)


def _check_forward(m, sc, rays, rk):
    """fused_march ids and features against the oracle (exact), then the model's dict against the float64 head."""
    from directvoxgo_amd.fused import fused_march
    ro, rd, vd = rays
    ref = R.forward(sc, _np(ro), _np(rd), _np(vd), dtype=torch.float64, **rk)
    with torch.no_grad():
        res = m(ro, rd, vd, render_depth=True, **rk)
        cfg = next(iter(m._cfg_cache.values()))
        _, _, _, feat, ray_id, step_id, _ = fused_march(m.density, m.k0, ro, rd, cfg)
    assert np.array_equal(_np(ray_id), ref['ray_id']) and np.array_equal(_np(res['ray_id']), ref['ray_id'])
    assert np.array_equal(_np(step_id), ref['step_id'])
    assert np.array_equal(_np(feat), ref['feat'])          # bit for bit: same trilinear setup and fmaf order
    np.testing.assert_allclose(_np(res['weights']), ref['weights'], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(_np(res['raw_alpha']), ref['raw_alpha'], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(_np(res['alphainv_last']), ref['alphainv_last'], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(_np(res['raw_rgb']), ref['raw_rgb'], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(_np(res['rgb_marched']), ref['rgb_marched'], atol=1e-5)
    _check_depth(_np(res['depth']), ref)
    return ref


def _check_depth(got, ref, what='depth'):
    """depth = sum of w * step_id: each weight carries the allowance above (rtol 1e-5, atol 1e-6), multiplied by step ids
    in the hundreds at these sizes, so the bound is that allowance summed along the ray (plus the golden test's own)."""
    bound = np.zeros_like(ref['depth'], dtype=np.float64)
    np.add.at(bound, ref['ray_id'], (1e-5 * ref['weights'] + 1e-6) * ref['step_id'])
    err = np.abs(got - ref['depth'])
    assert np.all(err <= bound + 1e-5 * np.abs(ref['depth']) + 1e-4), (what, float((err - bound).max()))


def _check_gradients(m, sc, ref, target, n_rays, rk):
    """fused_render_loss(FINE_TRAIN) + backward on the GPU against the oracle chain with the float64 head."""
    from directvoxgo_amd.train import FINE_TRAIN, fused_render_loss
    ro, rd, vd = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in ref['_rays'])
    m.zero_grad(set_to_none=True)
    seen, shade = [], m._shade
    def tap(k0, *a, **kw):                                 # the head's per-sample feature gradient, as autograd passes it
        if k0.requires_grad:
            k0.register_hook(lambda g: seen.append(g.detach().clone()))
        return shade(k0, *a, **kw)
    m._shade = tap
    # beside the grid-wide `_within` below: every record of every ray against tests/march_oracle.py, on the launches' own arguments
    with MO.MarchSpy() as spy:
        try:
            res = m(ro, rd, vd, **rk)
        finally:
            m._shade = shade
        loss = fused_render_loss(res, target, n_rays, dict(FINE_TRAIN))
        loss.backward()
        torch.cuda.synchronize()
    summ = spy.summary()
    assert summ['march_density'][0] == 1 and summ['march_density_bwd'][0] == 1 and summ['march_density_bwd'][1] == summ['march_density'][1]
    print('march per sample (launches, elements, worst err / bound)', summ)
    ref_loss, g = R.loss_and_grads(sc, ref, _np(target), w_main=FINE_TRAIN['weight_main'],
                                   w_ent=FINE_TRAIN['weight_entropy_last'], w_per=FINE_TRAIN['weight_rgbper'])
    np.testing.assert_allclose(float(loss.detach()), ref_loss, rtol=1e-5)
    # colour head data gradient per sample.  A hidden unit whose float64 pre-activation lies within a float32 dot product's
    # worst-case rounding of zero (128 terms: 128 * 2^-24 < 1e-5 of the terms' magnitudes) may take the other ReLU branch
    # in the kernel; that sample then has another, equally valid, feature gradient.  Every sample that disagrees must be
    # such a tie, and they must be rare (15 of 2 M at the roofline size); only they take the GPU's value below
    g_feat = _np(seen[0])
    bad = np.abs(g_feat - g['g_feat']).max(1) > 2e-4 * np.abs(g['g_feat']).max()
    margin = R.relu_margin(sc, ref)
    assert bad.mean() < 1e-4 and np.all(margin[bad] < 1e-5), (int(bad.sum()), margin[bad].max(initial=0))
    want_feat = np.where(bad[:, None], g_feat, g['g_feat'])
    g['grad_k0'] = oracle_scatter(want_feat, sc, ref)
    gd, gk = _np(m.density.grad)[0, 0], _np(m.k0.grad)[0]
    for a, b, what in ((gd, g['grad_density'], 'density'), (gk, g['grad_k0'], 'k0')):
        _within(a, b, 1e-4, what)                          # summation order of the scatter, nothing else
        assert np.array_equal(a != 0, b != 0), what        # same touched voxels
    for k, p in m.rgbnet.named_parameters():               # 2 M-row weight-gradient sums against float64
        _within(_np(p.grad), g['grad_rgbnet_' + k], 2e-4, k)
    return g


def oracle_scatter(g_feat, sc, ref):
    from oracle import oracle as O
    return O.grid_sample_bwd(g_feat, sc.k0.shape, ref['pts'], sc.xyz_min, sc.xyz_max)


def _rays_of(ref, ro, rd, vd):
    ref['_rays'] = (_np(ro), _np(rd), _np(vd))
    return ref


def _roofline_model():
    from directvoxgo_amd.dvgo import DirectVoxGO
    from directvoxgo_amd.scenes import roofline_scene
    scn = roofline_scene(world=160, n_rays=8192, device='cuda')
    torch.manual_seed(0)
    m = DirectVoxGO(scn['xyz_min'], scn['xyz_max'], num_voxels=160 ** 3, num_voxels_base=160 ** 3, alpha_init=1e-2,
                    fast_color_thres=1e-4, rgbnet_dim=12, rgbnet_width=128, rgbnet_direct=True).cuda()
    with torch.no_grad():
        m.density.copy_(scn['density']); m.k0.copy_(scn['k0'])
    return scn, m


@pytest.mark.timeout(600)
def test_roofline_160_cubed_matches_the_oracle(oracle):
    from directvoxgo_amd.fused import fused_march
    scn, m = _roofline_model()
    assert m.k0.stride()[1] == 1
    sc = _host_scene(m)
    rk = dict(near=scn['near'], far=scn['far'], bg=1, stepsize=0.5)
    rays = (scn['rays_o'], scn['rays_d'], scn['viewdirs'])
    ref = _rays_of(_check_forward(m, sc, rays, rk), *rays)
    assert ref['weights'].shape[0] == 8192 * 256
    _check_gradients(m, sc, ref, scn['target'], 8192, rk)
    # the scatter alone: the GPU's own per-sample feature gradient through the oracle's grid_sample_bwd
    m.zero_grad(set_to_none=True)
    _, _, _, feat, ray_id, step_id, _ = fused_march(m.density, m.k0, *rays[:2], m._march_cfg(**{k: rk[k] for k in ('near', 'far', 'stepsize')}))
    g_feat = torch.randn(feat.shape, device='cuda', generator=torch.Generator(device='cuda').manual_seed(3))
    feat.backward(g_feat)
    want = oracle.grid_sample_bwd(_np(g_feat), tuple(m.k0.shape[1:]), ref['pts'], sc.xyz_min, sc.xyz_max)
    np.testing.assert_allclose(_np(m.k0.grad)[0], want, rtol=1e-4, atol=1e-6 * np.abs(want).max())


@pytest.mark.timeout(600)
def test_lego_like_160_cubed_matches_the_oracle_and_takes_the_reference_adam_step(oracle):
    from directvoxgo_amd.dvgo import DirectVoxGO
    from directvoxgo_amd.scenes import synthetic_scene
    from directvoxgo_amd.train import FINE_TRAIN, TrainStep
    scn = synthetic_scene(world=160, n_rays=8192, device='cuda')
    torch.manual_seed(1)
    m = DirectVoxGO(scn['xyz_min'], scn['xyz_max'], num_voxels=160 ** 3, num_voxels_base=160 ** 3, alpha_init=1e-2,
                    fast_color_thres=1e-4, rgbnet_dim=12, rgbnet_width=128, rgbnet_direct=True).cuda()
    with torch.no_grad():
        m.density.copy_(scn['density']); m.k0.copy_(scn['k0']); m.mask_cache.mask.copy_(scn['mask'])
    sc = _host_scene(m)
    rk = dict(near=scn['near'], far=scn['far'], bg=1, stepsize=scn['stepsize'])
    rays = (scn['rays_o'], scn['rays_d'], scn['viewdirs'])
    ref = _rays_of(_check_forward(m, sc, rays, rk), *rays)
    assert 0 < ref['weights'].shape[0] < 8192 * 256 and (ref['alphainv_last'] < 1e-3).any()    # culled, terminated
    hit = R.hit_coarse_geo(sc, _np(rays[0]), _np(rays[1]), rk['near'], rk['far'], rk['stepsize'])
    assert 0 < hit.sum() < hit.size
    assert np.array_equal(_np(m.hit_coarse_geo(rays_o=rays[0], rays_d=rays[1], **rk)), hit)
    g = _check_gradients(m, sc, ref, scn['target'], 8192, rk)

    # one training step on the capacity path (Adam fused into the brick kernel) = oracle Adam from zero moments
    p0 = {'density': _np(m.density)[0, 0], 'k0': _np(m.k0)[0]}
    p0.update({k: _np(p) for k, p in m.rgbnet.named_parameters()})
    m.zero_grad(set_to_none=True)
    step = TrainStep(m, dict(FINE_TRAIN), rk, sync_free=True)          # counts stay on the device
    step(*rays, scn['target'], global_step=1)
    torch.cuda.synchronize()
    assert m.density.grad is None and m.k0.grad is None and step.last_fused_adam       # the fused update ran
    got = {'density': _np(m.density)[0, 0], 'k0': _np(m.k0)[0]}
    got.update({k: _np(p) for k, p in m.rgbnet.named_parameters()})
    lr = {'density': FINE_TRAIN['lrate_density'], 'k0': FINE_TRAIN['lrate_k0']}
    for name, p in p0.items():
        grad = g['grad_' + name] if name in lr else g['grad_rgbnet_' + name].astype(np.float32)
        want = np.ascontiguousarray(p, np.float32).copy()
        grad = np.ascontiguousarray(grad, np.float32)
        oracle.adam_upd(want, grad, np.zeros_like(want), np.zeros_like(want), 1, 0.9, 0.99,
                        lr.get(name, FINE_TRAIN['lrate_rgbnet']), 1e-8, mode=1 if name in lr else 0)
        if name in lr:
            # the set of updated voxels (masked Adam: grad != 0) is that of the oracle's gradients, up to a sum of a few
            # terms that cancels to exactly 0.0f in one summation order and not in the other (the allowance of
            # test_gpu_brick.py::test_adam_fused_into_the_brick_kernel_equals_dense_gradients_plus_masked_adam)
            n_diff = int(((got[name] != p) != (want != p)).sum())
            assert n_diff <= 1e-6 * p.size + 2, (name, n_diff)
            # a first Adam step moves by ~lr * sign(grad).  Where |grad| is below the gradients' own comparison bound
            # (1e-4 max|grad|, summation order) the sign itself is not determined, so only those may differ by 2 lr
            d = np.abs(got[name] - want)
            firm = np.abs(grad) > 2e-4 * np.abs(grad).max()
            assert float(d[firm].max()) <= 2e-3, name
            assert float((d > 2e-3).mean()) <= 1e-3 and float(d.max()) <= 2 * lr[name] + 2e-3, name
        else:
            np.testing.assert_allclose(got[name], want, atol=5e-5, err_msg=name)


@pytest.mark.timeout(600)
def test_config5_render_slices_match_the_oracle():
    from directvoxgo_amd.render import get_rays_of_a_view, render_viewpoints
    from directvoxgo_amd.scenes import pose_spherical
    from test_gpu_configs import _truck_like_model
    scn, m = _truck_like_model(256)
    assert m.k0.numel() * 4 > 800e6 and m.k0.stride()[1] == 1
    H = W = 800
    K = np.array([[1111.11, 0, 0.5 * W], [0, 1111.11, 0.5 * H], [0, 0, 1]], np.float32)
    pose = pose_spherical(35.0, -30.0, 4.0)
    pose[:3, 1] *= -1; pose[:3, 2] *= -1                                     # OpenCV convention: inverse_y
    rk = dict(near=0.0, far=8.0, bg=1, stepsize=0.5, inverse_y=True, flip_x=False, flip_y=False)
    rgbs, depths = render_viewpoints(m, [pose.numpy()], [(H, W)], [K], False, rk)
    rgb, depth = rgbs[0].reshape(-1, 3), depths[0].reshape(-1)
    ro, rd, vd = (_np(t.flatten(0, -2)) for t in
                  get_rays_of_a_view(H, W, K, pose.cuda(), False, inverse_y=True, flip_x=False, flip_y=False))
    sc = _host_scene(m)
    del m
    torch.cuda.empty_cache()
    row = 400 * W
    cols = np.nonzero(depth[row:row + W] > 0)[0]
    assert 0 < cols.size < W
    starts = {'centre row': row + W // 2 - 1024, 'corner': 0, 'silhouette': row + int(cols[0]) - 1024}
    for what, s in starts.items():
        sl = slice(s, s + 2048)
        ref = R.forward(sc, ro[sl], rd[sl], vd[sl], near=0.0, far=8.0, stepsize=0.5, bg=1, dtype=torch.float64)
        np.testing.assert_allclose(rgb[sl], ref['rgb_marched'], atol=1e-5, err_msg=what)
        _check_depth(depth[sl], ref, what)
        if what == 'silhouette':
            assert 0 < (ref['depth'] > 0).sum() < 2048                      # both object and background pixels


@pytest.mark.timeout(600)
def test_config4_mpi_matches_the_oracle_with_dense_tv(oracle):
    from test_gpu_configs import _fern_like, _fern_rays
    m = _fern_like(True)
    assert m.world_size.tolist() == [343, 382, 128] and m.k0.shape[1] == 9 and m.k0.stride()[1] == 1
    ro, rd, vd, tgt = _fern_rays()
    sc = _host_scene(m)
    rk = dict(near=0, far=1, bg=0, stepsize=0.5)
    ref = _rays_of(_check_forward(m, sc, (ro, rd, vd), rk), ro, rd, vd)
    assert ref['weights'].shape[0] > 4096 * 20
    _check_gradients(m, sc, ref, tgt, 4096, rk)
    # dense TV with the llff weights (configs/llff/llff_default.py: 1e-5 over the batch) on both grids
    w = 1e-5 / 4096
    wxy, wz = w * float(m.world_size[:2].max()) / 128, w * m.mpi_depth / 128
    for name, add in (('density', m.density_total_variation_add_grad), ('k0', m.k0_total_variation_add_grad)):
        p = getattr(m, name)
        param = np.ascontiguousarray(_np(p))                   # the oracle's channels-first copy
        want = np.ascontiguousarray(_np(p.grad))
        oracle.total_variation_add_grad(param, want, wxy, wxy, wz, True)
        add(w, True)
        assert np.array_equal(_np(p.grad), want), name
