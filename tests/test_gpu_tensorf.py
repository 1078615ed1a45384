"""GPU: TensoRFVoxGO (directvoxgo_amd/tensorf.py) end to end on `synthetic_scene(world=32, n_rays=2048)`: its density against
the oracle and the float64 restatement at the render's own samples, the render, the gradients, the training step, a
checkpoint, scale_volume_grid, fit_stage's density_offset schedule, the near-camera mask, the ray samplers and the four
density regulariser keys.

The density is one that the decomposition represents exactly: component 0 of plane xy holds amp * exp(-(y^2 + z^2) / s^2)
and component 0 of its line (along x) exp(-x^2 / s^2), a separable Gaussian blob of raw density `amp` at the centre;
everything else is 0.01 * randn.  density_offset = -9 keeps the space around the blob empty."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import triplane_oracle as TO
import vm_density_oracle as DO
import vm_oracle as VO

pytestmark = pytest.mark.gpu

AMP, SIGMA, OFFSET = 20.0, 0.6, -9.0


@pytest.fixture(scope='module')
def scene():
    from directvoxgo_amd.scenes import synthetic_scene
    return synthetic_scene(world=32, n_rays=2048, seed=6, device='cuda')


def _rk(sc, **kw):
    return dict(near=sc['near'], far=sc['far'], bg=1, stepsize=0.5, **kw)


def _scene_model(sc, seed=1, **kw):
    from directvoxgo_amd.tensorf import TensoRFVoxGO
    torch.manual_seed(seed)
    m = TensoRFVoxGO(sc['xyz_min'], sc['xyz_max'], **{**dict(
        num_voxels=sc['world'] ** 3, num_voxels_base=sc['world'] ** 3, alpha_init=1e-2, fast_color_thres=1e-4, n_comp=8,
        density_n_comp=4, density_offset=OFFSET, rgbnet_dim=6, rgbnet_width=64), **kw})
    for p in m.rgbnet.parameters():
        torch.nn.init.normal_(p, std=0.1)
    m = m.cuda()
    with torch.no_grad():
        for p in list(m.density_planes.values()) + list(m.density_lines.values()):
            p.mul_(0.1)                                                              # 0.1 * randn -> 0.01 * randn
        pl, ln = m.density_planes['xy'], m.density_lines['xy']
        ax = [torch.linspace(float(sc['xyz_min'][a]), float(sc['xyz_max'][a]), n, device='cuda')
              for a, n in ((1, pl.shape[2]), (2, pl.shape[3]), (0, ln.shape[2]))]
        pl[0, 0] = AMP * torch.exp(-(ax[0][:, None] ** 2 + ax[1][None, :] ** 2) / SIGMA ** 2)      # rows y, columns z
        ln[0, 0, :, 0] = torch.exp(-ax[2] ** 2 / SIGMA ** 2)                                       # along x
    return m


def _np(d):
    return {k: p.detach().cpu().contiguous().numpy() for k, p in d.items()}


def test_raw_density_on_the_renders_own_samples(scene):
    """Against the oracle inside the forward bound (3R + 12) U A, every sample; and against the float64 torch restatement
    at the sampler's standing tolerances, rtol 1e-5 / atol 1e-6 (the positions are not dyadic: float32 coordinates differ
    from float64 ones by a few 1e-6 cells, and a cell changes the value by at most a quarter of it here)."""
    sc = scene
    m = _scene_model(sc)
    with torch.no_grad():
        pts, ray_id, _ = m.sample_ray(rays_o=sc['rays_o'], rays_d=sc['rays_d'], **_rk(sc))
        pts = pts[m.mask_cache(pts)]
        got = m.raw_density(pts)
    assert got.shape == (pts.shape[0],) and pts.shape[0] > 50000
    planes, lines, xyz = _np(m.density_planes), _np(m.density_lines), pts.cpu().numpy()
    mn, mx = m._xyz_min_cpu.numpy(), m._xyz_max_cpu.numpy()
    val, A = DO.forward(planes, lines, xyz, mn, mx)
    err = np.abs(got.cpu().numpy().astype(np.float64) - val)
    print('worst err / bound', float((err / np.maximum(DO.forward_bound(4, A), 1e-300)).max()), 'peak', float(val.max()))
    assert (err <= DO.forward_bound(4, A)).all() and val.max() > 0.5 * AMP
    t64 = lambda d: {k: torch.from_numpy(v).double() for k, v in d.items()}          # noqa: E731
    ref = VO.torch_restatement(t64(planes), t64(lines), torch.from_numpy(xyz).double(), torch.from_numpy(mn).double(),
                               torch.from_numpy(mx).double()).sum(-1).numpy()
    print('worst |got - restatement| / (1e-6 + 1e-5 |ref|)',
          float((np.abs(got.cpu().numpy() - ref) / (1e-6 + 1e-5 * np.abs(ref))).max()))
    np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=1e-5, atol=1e-6)


def test_render_sees_the_blob_and_gradients_reach_everything(scene):
    sc = scene
    m = _scene_model(sc)
    args = (sc['rays_o'], sc['rays_d'], sc['viewdirs'])
    res = m(*args, render_depth=True, **_rk(sc))
    assert set(res) == {'alphainv_last', 'weights', 'rgb_marched', 'raw_alpha', 'raw_rgb', 'ray_id', 'depth'}
    assert res['rgb_marched'].shape == (2048, 3) and res['ray_id'].shape[0] > 1000
    assert float((res['rgb_marched'].detach() - 1).abs().max()) > 0.05               # bg = 1
    assert float(res['alphainv_last'].detach().min()) < 0.5 and float(res['alphainv_last'].detach().max()) > 0.99   # through and beside it
    (res['rgb_marched'] - sc['target']).pow(2).mean().backward()
    for name, p in list(m.density_planes.items()) + list(m.density_lines.items()) + list(m.planes.items()) + \
            list(m.lines.items()) + [('basis', m.basis)] + list(m.rgbnet.named_parameters()):
        assert p.grad is not None and float(p.grad.abs().sum()) > 0, name
        assert p.grad.shape == p.shape
    # the caller's density tensors: rendered instead of the model's own, and the gradient goes to them
    m.zero_grad(set_to_none=True)
    feats = {**{k: p.detach() for k, p in m.planes.items()},
             'xy_density': (m.density_planes['xy'].detach() * 0.5).requires_grad_(),
             'xy_density_line': m.density_lines['xy'].detach().clone().requires_grad_()}
    ext = m.render(feats, *args, **_rk(sc))['rgb_marched']
    assert not torch.equal(ext, res['rgb_marched'])
    ext.sum().backward()
    assert float(feats['xy_density'].grad.abs().sum()) > 0 and float(feats['xy_density_line'].grad.abs().sum()) > 0
    assert m.density_planes['xy'].grad is None and float(m.density_planes['yz'].grad.abs().sum()) > 0


def test_train_step_checkpoint_and_scale_volume_grid(scene, tmp_path):
    from directvoxgo_amd.checkpoint import load_model, save_checkpoint
    from directvoxgo_amd.tensorf import TENSORF_FINE_TRAIN, TensoRFVoxGO
    from directvoxgo_amd.train import TrainStep
    sc = scene
    rk = _rk(sc)
    m = _scene_model(sc)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    step = TrainStep(m, dict(TENSORF_FINE_TRAIN), rk)
    assert not step.can_capture() and not m.can_keep_count_on_device()
    args = (sc['rays_o'], sc['rays_d'], sc['viewdirs'], sc['target'])
    losses = [float(step(*args, global_step=s)) for s in (1, 2, 3)]
    print('losses', losses)
    assert losses[2] < losses[0]
    after = m.state_dict()
    assert 'density' not in after
    for k in ('density_planes.xy', 'density_planes.yz', 'density_planes.zx', 'density_lines.xy', 'density_lines.yz',
              'density_lines.zx', 'planes.xy', 'planes.yz', 'planes.zx', 'lines.xy', 'lines.yz', 'lines.zx', 'basis',
              'rgbnet.0.weight', 'rgbnet.3.bias'):
        assert not torch.equal(before[k], after[k]), k
    path = str(tmp_path / 'tensorf.tar')
    save_checkpoint(path, m, step.optimizer, 3)
    m2 = load_model(TensoRFVoxGO, path).cuda()
    assert m2.density_n_comp == 4 and m2.density_offset == OFFSET and m2.density is None
    assert set(m2.state_dict()) == set(after) and all(torch.equal(v, m2.state_dict()[k]) for k, v in after.items())
    with torch.no_grad():
        ra, rb = m(*args[:3], render_depth=True, **rk), m2(*args[:3], render_depth=True, **rk)
    assert all(torch.equal(ra[k], rb[k]) for k in ('rgb_marched', 'depth', 'weights', 'ray_id'))

    old = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m.scale_volume_grid(40 ** 3)
    ws = tuple(int(v) for v in m.world_size)
    assert min(ws) > 32 and tuple(m.mask_cache.mask.shape) == ws and m.density is None
    for k in VO.KEYS:
        hw = (ws[TO.AXES[k][0]], ws[TO.AXES[k][1]])
        p, ln = m.density_planes[k], m.density_lines[k]
        ref = F.interpolate(old['density_planes.' + k].contiguous(), size=hw, mode='bilinear', align_corners=True)
        assert tuple(p.shape) == (1, 4, *hw) and p.stride(1) == 1 and torch.equal(p.detach(), ref)
        n = ws[VO.LINE_AXIS[k]]
        ref = F.interpolate(old['density_lines.' + k].contiguous(), size=(n, 1), mode='bilinear', align_corners=True)
        assert tuple(ln.shape) == (1, 4, n, 1) and ln.stride(1) == 1 and torch.equal(ln.detach(), ref)
        assert tuple(m.planes[k].shape) == (1, 8, *hw) and tuple(m.lines[k].shape) == (1, 8, n, 1)
    mask = m.mask_cache.mask
    assert 0 < int(mask.sum()) < mask.numel() and torch.equal(mask, m._alpha_mask())       # rebuilt from dense_density()
    assert torch.isfinite(m(*args[:3], **rk)['rgb_marched']).all()
    fixed = _scene_model(sc, density_plane_size=(20, 24), density_line_size=11)
    held = {k: v.detach().clone() for k, v in fixed.state_dict().items() if k.startswith('density_')}
    fixed.scale_volume_grid(40 ** 3)
    assert len(held) == 6 and all(torch.equal(v, fixed.state_dict()[k]) for k, v in held.items())
    assert tuple(fixed.mask_cache.mask.shape) == ws and tuple(fixed.planes['xy'].shape) == (1, 8, ws[1], ws[2])


def test_fit_stage_lowers_the_offset_at_a_pg_scale_step(scene):
    from directvoxgo_amd.fit import fit_stage
    from directvoxgo_amd.tensorf import TENSORF_FINE_TRAIN
    sc = scene
    m = _scene_model(sc)
    cfg = dict(TENSORF_FINE_TRAIN, pg_scale=[2], N_rand=1024)
    psnr = fit_stage(m, sc['rays_o'], sc['rays_d'], sc['viewdirs'], sc['target'], cfg, _rk(sc), n_iters=4,
                     num_voxels_final=sc['world'] ** 3)
    assert len(psnr) == 4 and all(np.isfinite(psnr))
    assert m.density_offset == OFFSET - 1.0 and m.get_kwargs()['density_offset'] == OFFSET - 1.0
    assert m.num_voxels == sc['world'] ** 3 and m.density is None
    assert tuple(m.mask_cache.mask.shape) == tuple(int(v) for v in m.world_size)


def test_maskout_near_cam_vox_clears_the_mask_where_dvgo_writes_minus_100(scene):
    from directvoxgo_amd.dvgo import DirectVoxGO
    sc = scene
    m = _scene_model(sc)
    d = DirectVoxGO(sc['xyz_min'], sc['xyz_max'], num_voxels=sc['world'] ** 3, num_voxels_base=sc['world'] ** 3,
                    alpha_init=1e-2).cuda()
    cams = np.float32([[1.2, 1.0, -0.9], [-1.5, 0.1, 0.2], [4.0, 4.0, 4.0]])
    assert bool(m.mask_cache.mask.all())
    m.maskout_near_cam_vox(cams, 0.45)
    d.maskout_near_cam_vox(cams, 0.45)
    gone = d.density.detach()[0, 0] == -100
    assert 0 < int(gone.sum()) < gone.numel() and torch.equal(~m.mask_cache.mask, gone)
    m.maskout_near_cam_vox(cams[:1], 0.2)                                            # a second call only clears more
    assert torch.equal(~m.mask_cache.mask, gone)


def test_in_maskcache_rays_and_render_viewpoints(scene):
    """The 'in_maskcache' ray sampler keeps the rays `hit_coarse_geo` says cross occupied space: with the mask rebuilt from
    the model's own density those are the rays that can see the blob, and every pixel that does not render as background is
    among them.  render_viewpoints returns the model's own render."""
    from directvoxgo_amd.render import get_rays_of_a_view, get_training_rays_in_maskcache_sampling, render_viewpoints
    from directvoxgo_amd.scenes import pose_spherical
    sc = scene
    m = _scene_model(sc)
    with torch.no_grad():
        m._set_mask_cache(m._alpha_mask())
    assert 0 < int(m.mask_cache.mask.sum()) < m.mask_cache.mask.numel()
    H = W = 16
    K = np.array([[20.0, 0, 0.5 * W], [0, 20.0, 0.5 * H], [0, 0, 1]], np.float32)
    poses = [pose_spherical(30.0, -30.0, 4.0), pose_spherical(-100.0, -20.0, 4.0)]
    rk = _rk(sc, inverse_y=False)
    rgbs, depths = render_viewpoints(m, [p.numpy() for p in poses], [(H, W)] * 2, [K] * 2, False, rk)
    assert rgbs.shape == (2, H, W, 3) and depths.shape == (2, H, W, 1)
    own = []
    for i, pose in enumerate(poses):
        ro, rd, vd = get_rays_of_a_view(H, W, K, pose.cuda(), False, False, False, False)
        with torch.no_grad():
            res = m(ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous(), vd.reshape(-1, 3).contiguous(),
                    render_depth=True, **rk)
        assert float((res['rgb_marched'] - 1).abs().max()) > 0.05                   # the view sees the blob
        np.testing.assert_allclose(rgbs[i].reshape(-1, 3), res['rgb_marched'].cpu().numpy(), atol=1e-6)
        np.testing.assert_allclose(depths[i].reshape(-1), res['depth'].cpu().numpy(), atol=1e-4)
        own.append(res['rgb_marched'].reshape(H, W, 3))
    imgs = [torch.rand(H, W, 3, device='cuda') for _ in poses]
    rgb, ro, rd, vd, imsz = get_training_rays_in_maskcache_sampling(
        imgs, [p.numpy() for p in poses], [(H, W)] * 2, [K] * 2, False, False, False, False, m,
        dict(near=sc['near'], far=sc['far'], stepsize=0.5))
    assert sum(imsz) == rgb.shape[0] == ro.shape[0] and 0 < imsz[0] < H * W
    top = 0
    for i, pose in enumerate(poses):
        o, d, _ = get_rays_of_a_view(H, W, K, pose.cuda(), False, False, False, False)
        hit = m.hit_coarse_geo(rays_o=o, rays_d=d, near=sc['near'], far=sc['far'], stepsize=0.5)
        assert int(hit.sum()) == imsz[i] and torch.equal(rgb[top:top + imsz[i]], imgs[i][hit])
        assert bool(hit[(own[i] - 1).abs().amax(-1) > 1e-6].all())                   # what is not background was hit
        top += imsz[i]


def test_density_regulariser_keys_give_the_hand_made_launch(scene):
    """What TrainStep does for the four keys (`_tv_add_grad`, inside the tv window) against ops.plane_reg_add_grad called by
    hand on the six density tensors with the documented weights, both on copies of the gradients of one backward (the
    scatter's float atomics make two backwards differ in their last bits): equal bit for bit, and the colour side is not
    touched."""
    from directvoxgo_amd.ops import plane_reg_add_grad
    from directvoxgo_amd.tensorf import TENSORF_FINE_TRAIN
    from directvoxgo_amd.train import TrainStep
    sc = scene
    keys = dict(weight_tv_density_planes=1e-2, weight_tv_density_lines=2e-2, weight_l1_density_planes=3e-3,
                weight_l1_density_lines=4e-3)
    cfg = dict(TENSORF_FINE_TRAIN, tv_after=0, tv_before=100, tv_every=1, tv_dense_before=100, **keys)
    n = sc['rays_o'].shape[0]
    m = _scene_model(sc)
    step = TrainStep(m, cfg, _rk(sc))
    assert step.density_reg_on and not step.plane_reg_on
    assert step._plan(sc['rays_o'], 1).tv and not step._plan(sc['rays_o'], 100).tv          # the usual window
    res = m(sc['rays_o'], sc['rays_d'], sc['viewdirs'], global_step=1, **_rk(sc))
    (res['rgb_marched'] - sc['target']).pow(2).mean().backward()
    g0 = {name: p.grad.detach().clone(memory_format=torch.preserve_format) for name, p in m.named_parameters()}

    step._tv_add_grad(1, n)
    by_step = {name: p.grad.detach().clone() for name, p in m.named_parameters()}

    for name, p in m.named_parameters():
        p.grad = g0[name].clone(memory_format=torch.preserve_format)
    ps = list(m.density_planes.values()) + list(m.density_lines.values())
    ws = [(keys['weight_tv_density_planes'] / n * max(p.shape[2], p.shape[3]) / 128 / 4,) * 2
          + (keys['weight_l1_density_planes'] / n,) for p in m.density_planes.values()]
    ws += [(keys['weight_tv_density_lines'] / n * p.shape[2] / 128 / 2, 0.0, keys['weight_l1_density_lines'] / n)
           for p in m.density_lines.values()]
    plane_reg_add_grad([p.detach() for p in ps], [p.grad for p in ps], ws, True)
    changed = 0
    for name, p in m.named_parameters():
        assert torch.equal(by_step[name], p.grad), name
        if name.startswith('density_'):
            assert not torch.equal(by_step[name], g0[name]), name
            changed += 1
        else:
            assert torch.equal(by_step[name], g0[name]), name
    assert changed == 6
