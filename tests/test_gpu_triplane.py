"""GPU: the tri-plane sampler (csrc/triplane.hip) against the float64 oracle of tests/triplane_oracle.py on every output
and every texel, and TriPlaneVoxGO against the reference fixtures of tests/golden/make_golden_triplane.py, fused against
unfused, with external planes, through the training step, a checkpoint and scale_volume_grid.

Error bounds (u = 2^-24; A = the sum of the |terms| of a result), derived, not tuned:
  forward   |got - exp| <= (T + 1) u A: the weights are the oracle's float32 numbers, each of the T fused multiply-adds of
            a chain rounds once (T = 4 per plane; 'sum' adds the three chains: T = 12 covers its 14 roundings' first-order
            bound of 6 u A as well);
  backward  |got - exp| <= (n + 2) u A per texel with n contributions, for any order of the atomics and of a lane's own
            run sums: each product w * g rounds once (u A in all), and n - 1 additions round once each on a partial sum of
            at most A;
  a texel with no contribution is exactly 0.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden

import triplane_oracle as TO

pytestmark = pytest.mark.gpu

AGGS = ('concat', 'sum')
SIZES = ({'xy': (6, 7), 'yz': (3, 9), 'zx': (8, 2)},            # different, non-square
         {'xy': (1, 5), 'yz': (33, 4), 'zx': (2, 2)})           # an axis of size 1; 33 rows: 5 % outside drops all four corners
MN, MX = np.array([-1.0, -0.8, -0.6], np.float32), np.array([0.9, 1.1, 0.7], np.float32)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def points(M, sizes, rng):
    """Up to 5 % outside the box; the box corners first, then texel centres of each plane."""
    xyz = (rng.random((M, 3)) * (MX - MN) * 1.1 + MN - 0.05 * (MX - MN)).astype(np.float32)
    special = [[(MN, MX)[(i >> a) & 1][a] for a in range(3)] for i in range(8)]
    for key, (H, W) in sizes.items():
        ah, aw = TO.AXES[key]
        for i in range(6):
            p = (MN + (MX - MN) * rng.random(3)).astype(np.float32)
            p[ah] = MN[ah] + (MX[ah] - MN[ah]) * np.float32((i % H) / max(H - 1, 1))
            p[aw] = MN[aw] + (MX[aw] - MN[aw]) * np.float32((i % W) / max(W - 1, 1))
            special.append(p)
    special = np.array(special, np.float32)[:M]
    xyz[:len(special)] = special
    return xyz


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


@pytest.mark.parametrize('layout', ['cf', 'cl', 'off'])
@pytest.mark.parametrize('C', [1, 3, 4, 12, 32])
def test_sampler_against_oracle(C, layout):
    from directvoxgo_amd.ops import triplane_bwd, triplane_fwd
    rng = np.random.default_rng(1000 * C + len(layout))
    mn, mx = cu(MN), cu(MX)
    worst_f = worst_b = 0.0
    for sizes in SIZES:
        planes = {k: rng.standard_normal((1, C, *hw)).astype(np.float32) for k, hw in sizes.items()}
        dev = {k: lay_out(p, layout) for k, p in planes.items()}
        shapes = {k: p.shape[1:] for k, p in planes.items()}
        for M in (0, 1, 63, 64, 65, 1000):
            xyz = points(M, sizes, rng)
            for agg in AGGS:
                T = 4 if agg == 'concat' else 12
                got = triplane_fwd(dev, cu(xyz), mn, mx, agg).cpu().numpy().astype(np.float64)
                exp, A = TO.forward(planes, xyz, MN, MX, agg)
                assert got.shape == exp.shape == (M, 3 * C if agg == 'concat' else C)
                err = np.abs(got - exp)
                bound = (T + 1) * TO.U * A
                assert (err <= bound).all(), (sizes, M, agg, float((err - bound).max()))
                if M:
                    worst_f = max(worst_f, float((err / np.maximum(bound, 1e-300)).max()))
                gout = rng.standard_normal(exp.shape).astype(np.float32)
                ref = TO.backward(shapes, xyz, MN, MX, gout, agg)
                for run in (0, 1, 8):
                    grads = {k: lay_out(np.zeros_like(p), layout) for k, p in planes.items()}
                    triplane_bwd(cu(gout), grads, cu(xyz), mn, mx, agg, run=run)
                    for k in TO.KEYS:
                        g, Ag, n = ref[k]
                        gg = grads[k][0].cpu().numpy().astype(np.float64)
                        err = np.abs(gg - g)
                        bound = (n[None] + 2) * TO.U * Ag
                        assert (err <= bound).all(), (sizes, M, agg, run, k, float((err - bound).max()))
                        assert (gg[:, n == 0] == 0).all(), (sizes, M, agg, run, k)
                        if M:
                            worst_b = max(worst_b, float((err / np.maximum(bound, 1e-300)).max()))
    print(f'C={C} {layout}: worst forward err / bound {worst_f:.3f}, worst backward err / bound {worst_b:.3f}')


def test_sampler_accumulates_into_the_callers_buffers():
    from directvoxgo_amd.ops import triplane_bwd
    rng = np.random.default_rng(5)
    sizes, C, M = SIZES[0], 4, 200
    xyz = points(M, sizes, rng)
    gout = rng.standard_normal((M, 3 * C)).astype(np.float32)
    start = {k: rng.standard_normal((1, C, *hw)).astype(np.float32) for k, hw in sizes.items()}
    grads = {k: lay_out(p, 'cl') for k, p in start.items()}
    triplane_bwd(cu(gout), grads, cu(xyz), cu(MN), cu(MX), 'concat')
    ref = TO.backward({k: p.shape[1:] for k, p in start.items()}, xyz, MN, MX, gout, 'concat')
    for k in TO.KEYS:
        g, Ag, n = ref[k]
        err = np.abs(grads[k][0].cpu().numpy().astype(np.float64) - (g + start[k][0]))
        assert (err <= (n[None] + 3) * TO.U * (Ag + np.abs(start[k][0]))).all()         # one more term: the start value


@pytest.mark.parametrize('agg', AGGS)
def test_op_autograd_and_reference_fixture(agg):
    """triplane_sample on the reference's grid_sampler2D fixture at the sampler's standing tolerances (values rtol 1e-5 /
    atol 1e-6, gradients rtol 1e-4 / atol 1e-6), from channel-first planes (the samples outnumber the texels: the op hands
    the kernels channels-last copies), from channels-last ones and from a 3-sequence; no gradient for xyz."""
    from directvoxgo_amd.ops import triplane_sample
    z = load_golden('triplane')
    for layout in ('cf', 'cl'):
        planes = {k: lay_out(z['plane_' + k], layout).requires_grad_() for k in TO.KEYS}
        xyz = cu(z['xyz'])
        out = triplane_sample(planes if layout == 'cf' else [planes[k] for k in TO.KEYS], xyz, cu(z['xyz_min']), cu(z['xyz_max']), agg)
        np.testing.assert_allclose(out.detach().cpu().numpy(), z[agg + '_out'], rtol=1e-5, atol=1e-6)
        out.backward(cu(z[agg + '_gout']))
        for k in TO.KEYS:
            assert planes[k].grad.shape == planes[k].shape
            np.testing.assert_allclose(planes[k].grad.cpu().numpy(), z[f'{agg}_gplane_{k}'], rtol=1e-4, atol=1e-6)
    shaped = triplane_sample(planes, xyz.reshape(20, 20, 3), cu(z['xyz_min']), cu(z['xyz_max']), agg)
    assert shaped.shape == (20, 20, out.shape[1]) and torch.equal(shaped.reshape(400, -1), out)


# ---------------------------------------------------------------------------------------------- the model
def rk_of(g, depth=True):
    return dict(near=float(g['near']), far=float(g['far']), bg=int(g['bg']), stepsize=float(g['stepsize']),
                inverse_y=False, flip_x=False, flip_y=False, render_depth=depth)


def build_model(g, agg, fused):
    from directvoxgo_amd.triplane import TriPlaneVoxGO
    nv = int(np.prod(g['world_size']))
    m = TriPlaneVoxGO(g['xyz_min'], g['xyz_max'], num_voxels=nv, num_voxels_base=nv, alpha_init=1e-2,
                      fast_color_thres=float(g['fast_color_thres']), fused=fused, rgbnet_dim=int(g['rgbnet_dim']), rgbnet_depth=3,
                      rgbnet_width=64, viewbase_pe=4, rgbnet_direct=False, tri_aggregation=agg)
    assert tuple(int(v) for v in m.world_size) == tuple(g['world_size'])
    with torch.no_grad():
        m.density.copy_(torch.from_numpy(g['density']))
        m.mask_cache.mask.copy_(torch.from_numpy(g['mask']))
        m.rgbnet.load_state_dict({k[len(agg) + len('_rgbnet_'):]: torch.from_numpy(v) for k, v in g.items()
                                  if k.startswith(agg + '_rgbnet_')})
    return m.cuda()


def loss_fn(res, target, n_rays, w_ent=0.001, w_per=0.01):
    """run.py:377-386"""
    loss = F.mse_loss(res['rgb_marched'], target)
    pout = res['alphainv_last'].clamp(1e-6, 1 - 1e-6)
    loss = loss + w_ent * (-(pout * torch.log(pout) + (1 - pout) * torch.log(1 - pout)).mean())
    rgbper = (res['raw_rgb'] - target[res['ray_id']]).pow(2).sum(-1)
    return loss + w_per * ((rgbper * res['weights'].detach()).sum() / n_rays)


def run_fixture(m, g):
    feats = {k: cu(g['plane_' + k]).requires_grad_() for k in TO.KEYS}
    ro, rd, vd = cu(g['rays_o']), cu(g['rays_d']), cu(g['viewdirs'])
    res = m.render(feats, ro, rd, vd, 0, **rk_of(g))
    loss = loss_fn(res, cu(g['target']), ro.shape[0])
    loss.backward()
    return res, loss, feats


@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('agg', AGGS)
def test_forward_matches_reference_orchestration(agg, fused):
    """The tolerances of test_gpu_posenc.test_forward_matches_reference_orchestration; the planes are the caller's
    (render(feats=...)): the gradients arrive there and model.planes stays without one."""
    g = load_golden('forward_triplane')
    m = build_model(g, agg, fused)
    res, loss, feats = run_fixture(m, g)
    p = agg + '_'
    assert np.array_equal(res['ray_id'].cpu().numpy(), g[p + 'out_ray_id'])
    np.testing.assert_allclose(res['weights'].detach().cpu().numpy(), g[p + 'out_weights'], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(res['raw_alpha'].detach().cpu().numpy(), g[p + 'out_raw_alpha'], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(res['alphainv_last'].detach().cpu().numpy(), g[p + 'out_alphainv_last'], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(res['raw_rgb'].detach().cpu().numpy(), g[p + 'out_raw_rgb'], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(res['rgb_marched'].detach().cpu().numpy(), g[p + 'out_rgb_marched'], atol=1e-5)
    np.testing.assert_allclose(res['depth'].cpu().numpy(), g[p + 'out_depth'], rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(float(loss), float(g[p + 'loss']), rtol=1e-5)
    np.testing.assert_allclose(m.density.grad.cpu().numpy(), g[p + 'grad_density'], rtol=1e-4, atol=1e-6)
    for k in TO.KEYS:
        np.testing.assert_allclose(feats[k].grad.cpu().numpy(), g[f'{p}grad_plane_{k}'], rtol=1e-4, atol=1e-6)
        assert m.planes[k].grad is None
    for k, q in m.rgbnet.named_parameters():
        np.testing.assert_allclose(q.grad.cpu().numpy(), g[p + 'grad_rgbnet_' + k], rtol=1e-3, atol=1e-6)


@pytest.mark.parametrize('agg', AGGS)
def test_fused_equals_unfused(agg):
    """Both paths call the same sampler on bit-equal positions: ray_id and the features are equal, and with the same
    colour head (torch's) behind them so are raw_rgb and rgb_marched."""
    from directvoxgo_amd.fused import fused_march
    g = load_golden('forward_triplane')
    outs, featv = {}, {}
    ro, rd, vd = cu(g['rays_o']), cu(g['rays_d']), cu(g['viewdirs'])
    planes = {k: cu(g['plane_' + k]) for k in TO.KEYS}
    rk = rk_of(g)
    for fused in (True, False):
        m = build_model(g, agg, fused)
        m.fused_shade = False
        with torch.no_grad():
            outs[fused] = m.render(planes, ro, rd, vd, **rk)
            if fused:
                cfg = m._march_cfg(rk['near'], rk['far'], rk['stepsize'])
                pts = fused_march(m.density, m.density.detach()[:, :0], ro, rd, cfg, positions=True)[3]
            else:
                pts, rid, sid = m.sample_ray(rays_o=ro, rays_d=rd, **rk)
                keep = m.mask_cache(pts)
                pts, rid = pts[keep], rid[keep]
                alpha = m.activate_density(m.grid_sampler(pts, m.density), rk['stepsize'] * m.voxel_size_ratio)
                pts, rid, alpha = pts[alpha > m.fast_color_thres], rid[alpha > m.fast_color_thres], alpha[alpha > m.fast_color_thres]
                from directvoxgo_amd.ops import Alphas2Weights
                w, _ = Alphas2Weights.apply(alpha, rid, ro.shape[0])
                pts = pts[w > m.fast_color_thres]
            featv[fused] = m.sample_planes(pts, planes)
    a, b = outs[True], outs[False]
    assert a['ray_id'].shape[0] > 100
    assert np.array_equal(a['ray_id'].cpu().numpy(), b['ray_id'].cpu().numpy())
    assert torch.equal(featv[True], featv[False])
    for k in ('weights', 'raw_alpha', 'alphainv_last', 'raw_rgb', 'rgb_marched', 'depth'):
        assert torch.equal(a[k], b[k]), k


def _scene_model(sc, agg='concat', plane_size=None, fused=True, world=None):
    from directvoxgo_amd.triplane import TriPlaneVoxGO
    w = world or sc['world']
    m = TriPlaneVoxGO(sc['xyz_min'], sc['xyz_max'], num_voxels=w ** 3, num_voxels_base=sc['world'] ** 3, alpha_init=1e-2,
                      fast_color_thres=1e-4, rgbnet_dim=4, rgbnet_width=64, tri_aggregation=agg, plane_size=plane_size, fused=fused)
    torch.manual_seed(1)
    for p in m.rgbnet.parameters():
        torch.nn.init.normal_(p, std=0.1)
    m = m.cuda()
    if w == sc['world']:
        with torch.no_grad():
            m.density.copy_(sc['density']); m.mask_cache.mask.copy_(sc['mask'])
    return m


def test_train_step_checkpoint_and_scale_volume_grid(tmp_path):
    """Three TrainStep steps on scenes.synthetic_scene lower the loss and move planes, density and MLP; a checkpoint
    written after them and loaded into a fresh model and optimizer gives an equal next step; scale_volume_grid resizes the
    planes that follow world_size and leaves fixed-size ones alone."""
    from directvoxgo_amd.checkpoint import load_checkpoint, load_model, save_checkpoint
    from directvoxgo_amd.scenes import synthetic_scene
    from directvoxgo_amd.train import TrainStep, create_optimizer_or_freeze_model
    from directvoxgo_amd.triplane import TRI_FINE_TRAIN, TriPlaneVoxGO
    sc = synthetic_scene(world=32, n_rays=2048, seed=6, device='cuda')
    cfg = dict(TRI_FINE_TRAIN)
    rk = dict(near=sc['near'], far=sc['far'], bg=1, stepsize=0.5)
    m = _scene_model(sc)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    step = TrainStep(m, cfg, rk)
    assert not step.can_capture()
    args = (sc['rays_o'], sc['rays_d'], sc['viewdirs'], sc['target'])
    losses = [float(step(*args, global_step=s)) for s in (1, 2, 3)]
    print('losses', losses)
    assert losses[2] < losses[0]
    after = m.state_dict()
    for k in ('density', 'planes.xy', 'planes.yz', 'planes.zx', 'rgbnet.0.weight', 'rgbnet.3.bias'):
        assert not torch.equal(before[k], after[k]), k
    path = str(tmp_path / 'tri.tar')
    save_checkpoint(path, m, step.optimizer, 3)
    m2 = load_model(TriPlaneVoxGO, path).cuda()
    assert m2.tri_aggregation == 'concat' and all(torch.equal(v, m2.state_dict()[k]) for k, v in m.state_dict().items())
    opt2 = create_optimizer_or_freeze_model(m2, cfg, global_step=0)
    _, opt2, gs = load_checkpoint(m2, opt2, path)
    assert gs == 3
    step2 = TrainStep(m2, cfg, rk, optimizer=opt2)
    la, lb = step(*args, global_step=4), step2(*args, global_step=4)
    np.testing.assert_allclose(float(la), float(lb), rtol=1e-6)
    for (k, p), q in zip(m.named_parameters(), m2.parameters()):          # (float atomics: Adam noise where a gradient is ~0)
        d = (p.detach() - q.detach()).abs()
        assert float((d > 2e-4).float().mean()) <= 1e-3 and float(d.max()) <= 0.11, k

    planes_before = {k: p.detach().clone() for k, p in m.planes.items()}
    m.scale_volume_grid(40 ** 3)
    X, Y, Z = ws = tuple(int(v) for v in m.world_size)
    assert min(ws) > 32 and tuple(m.density.shape[2:]) == ws
    for k, p in m.planes.items():
        hw = (ws[TO.AXES[k][0]], ws[TO.AXES[k][1]])
        ref = F.interpolate(planes_before[k].contiguous(), size=hw, mode='bilinear', align_corners=True)
        assert tuple(p.shape) == (1, 4, *hw) and p.stride(1) == 1 and torch.equal(p.detach(), ref)
    res = m(*args[:3], **rk)
    assert torch.isfinite(res['rgb_marched']).all()
    fixed = _scene_model(sc, plane_size=(20, 24))
    fixed.scale_volume_grid(40 ** 3)
    assert all(tuple(p.shape) == (1, 4, 20, 24) for p in fixed.planes.values()) and tuple(fixed.density.shape[2:]) == ws
