"""GPU: the positional-encoding colour head (posbase_pe > 0, csrc/shade_pe.hip) -- against the reference fixtures of
tests/golden/make_golden_posenc.py, against the float64 oracle of tests/posenc_oracle.py, and through the march, the
training step, mesh colouring and the renderer."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden

import posenc_oracle as PO

pytestmark = pytest.mark.gpu

FIXTURES = ('forward_fine_posenc', 'forward_fine_posenc_p4')


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def build_model(g, fused):
    from directvoxgo_amd.dvgo import DirectVoxGO
    nv = int(np.prod(g['world_size']))
    P = int(g['posbase_pe'])
    m = DirectVoxGO(g['xyz_min'], g['xyz_max'], num_voxels=nv, num_voxels_base=nv, alpha_init=1e-2,
                    fast_color_thres=float(g['fast_color_thres']), fused=fused, rgbnet_dim=12, rgbnet_depth=3,
                    rgbnet_width=128, viewbase_pe=4, rgbnet_direct=P == 10, posbase_pe=P)
    with torch.no_grad():
        m.density.copy_(torch.from_numpy(g['density']))
        m.k0.copy_(torch.from_numpy(g['k0']))
        m.mask_cache.mask.copy_(torch.from_numpy(g['mask']))
        m.rgbnet.load_state_dict({k[len('rgbnet_'):]: torch.from_numpy(v) for k, v in g.items() if k.startswith('rgbnet_')})
    return m.cuda()


def rk_of(g, depth=True):
    return dict(near=float(g['near']), far=float(g['far']), bg=int(g['bg']), stepsize=float(g['stepsize']),
                inverse_y=False, flip_x=False, flip_y=False, render_depth=depth)


def loss_fn(res, target, n_rays, w_ent=0.001, w_per=0.01):
    """run.py:377-386"""
    loss = F.mse_loss(res['rgb_marched'], target)
    pout = res['alphainv_last'].clamp(1e-6, 1 - 1e-6)
    loss = loss + w_ent * (-(pout * torch.log(pout) + (1 - pout) * torch.log(1 - pout)).mean())
    rgbper = (res['raw_rgb'] - target[res['ray_id']]).pow(2).sum(-1)
    return loss + w_per * ((rgbper * res['weights'].detach()).sum() / n_rays)


def run(m, g):
    ro, rd, vd = cu(g['rays_o']), cu(g['rays_d']), cu(g['viewdirs'])
    res = m(ro, rd, vd, global_step=0, **rk_of(g))
    loss = loss_fn(res, cu(g['target']), ro.shape[0])
    loss.backward()
    return res, loss


@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('name', FIXTURES)
def test_forward_matches_reference_orchestration(name, fused):
    """The tolerances of test_gpu_forward.test_forward_matches_reference_orchestration.  No extra allowance for P = 10:
    the head's positions are the reference's bit for bit (test_positions_equal_sample_ray), so its large arguments are
    the same float32 numbers on both sides."""
    from directvoxgo_amd.shade import posenc_supported
    g = load_golden(name)
    m = build_model(g, fused)
    assert posenc_supported(m.rgbnet, m.posbase_pe, 27)        # the HIP head is what runs in the fused path
    res, loss = run(m, g)
    assert np.array_equal(res['ray_id'].cpu().numpy(), g['out_ray_id'])
    np.testing.assert_allclose(res['weights'].detach().cpu().numpy(), g['out_weights'], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(res['raw_alpha'].detach().cpu().numpy(), g['out_raw_alpha'], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(res['alphainv_last'].detach().cpu().numpy(), g['out_alphainv_last'], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(res['raw_rgb'].detach().cpu().numpy(), g['out_raw_rgb'], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(res['rgb_marched'].detach().cpu().numpy(), g['out_rgb_marched'], atol=1e-5)
    np.testing.assert_allclose(res['depth'].cpu().numpy(), g['out_depth'], rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(float(loss), float(g['loss']), rtol=1e-5)
    assert m.k0.grad is None                                   # as in the reference: k0 is not part of the graph
    np.testing.assert_allclose(m.density.grad.cpu().numpy(), g['grad_density'], rtol=1e-4, atol=1e-6)
    for k, p in m.rgbnet.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), g['grad_rgbnet_' + k], rtol=1e-3, atol=1e-6)


@pytest.mark.parametrize('fused', [True, False])
def test_batch_in_which_no_sample_survives(fused):
    """Empty space everywhere (test_gpu_forward's case, for the positional-encoding model): no sample reaches the head,
    which must answer with an empty colour array and, after backward, no or zero parameter gradients.  The model then
    trains on a normal batch as if nothing had happened."""
    g = load_golden('forward_fine_posenc')
    m = build_model(g, fused)
    with torch.no_grad():
        m.density.fill_(-20.0)
    ro, rd, vd = cu(g['rays_o']), cu(g['rays_d']), cu(g['viewdirs'])
    res = m(ro, rd, vd, global_step=0, near=float(g['near']), far=float(g['far']), bg=1, stepsize=0.5, render_depth=True)
    assert res['weights'].numel() == 0 and res['raw_rgb'].shape == (0, 3)
    assert torch.allclose(res['rgb_marched'], torch.ones_like(res['rgb_marched']))      # pure background
    assert torch.all(res['alphainv_last'] == 1) and torch.all(res['depth'] == 0)
    loss_fn(res, cu(g['target']), ro.shape[0]).backward()
    assert m.density.grad is None or float(m.density.grad.abs().sum()) == 0.0
    for k, p in m.rgbnet.named_parameters():
        assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
    assert m.k0.grad is None
    # a normal batch next: the fixture's loss and gradients, to test_forward_matches_reference_orchestration's tolerances
    with torch.no_grad():
        m.density.copy_(torch.from_numpy(g['density']))
    m.zero_grad(set_to_none=True)
    res, loss = run(m, g)
    assert np.array_equal(res['ray_id'].cpu().numpy(), g['out_ray_id'])
    np.testing.assert_allclose(float(loss), float(g['loss']), rtol=1e-5)
    np.testing.assert_allclose(m.density.grad.cpu().numpy(), g['grad_density'], rtol=1e-4, atol=1e-6)
    for k, p in m.rgbnet.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), g['grad_rgbnet_' + k], rtol=1e-3, atol=1e-6)


def _head(P, seed, d_in=None):
    from directvoxgo_amd.dvgo import make_rgbnet
    torch.manual_seed(seed)
    net = make_rgbnet(d_in or (3 + 6 * P + 27), 128, 3)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(torch.randn_like(p) * 0.05)
    return net.cuda()


@pytest.mark.parametrize('P', [1, 4, 10])
def test_head_against_float64_oracle(P):
    """rgb and all six parameter gradients of the HIP head within the oracle's bounds: M ~ 2^17 plus an odd tail,
    positions up to +-1.5 (arguments up to 2^9 * 1.5 rad at P = 10).  Rows whose ReLU decisions are within rounding of
    a tie are dropped before the kernel sees the batch (tests/shade_oracle.py)."""
    from directvoxgo_amd.shade import defer_wgrad, shade_posenc, viewdir_embed
    gen = torch.Generator(device='cuda').manual_seed(100 + P)
    M0, R = 3 << 16, 4099                      # ~20 % of the rows are ReLU ties of this head: 2^17 + 75 are kept
    pts = (torch.rand((M0, 3), generator=gen, device='cuda') * 3 - 1.5).contiguous()
    vd = F.normalize(torch.randn((R, 3), generator=gen, device='cuda'), dim=-1).contiguous()
    ray_id = torch.randint(0, R, (M0,), generator=gen, device='cuda')
    freq = torch.tensor([2.0 ** i for i in range(P)], device='cuda')
    emb = viewdir_embed(vd, torch.tensor([1.0, 2.0, 4.0, 8.0], device='cuda'))
    net = _head(P, P)
    params = PO.params_of(net)
    _, _, margin = PO.forward(params, pts, freq, emb, ray_id)
    keep = PO.split_ties(margin)
    M = (1 << 17) + 75
    assert int(keep.sum()) >= M
    pts, ray_id = pts[keep][:M].contiguous(), ray_id[keep][:M].contiguous()
    g_rgb = torch.randn((M, 3), generator=gen, device='cuda')
    ref, mags = PO.forward_backward(params, pts, freq, emb, ray_id, g_rgb)
    for deferred in (False, True):
        net.zero_grad(set_to_none=True)
        if deferred:                         # the weight-gradient kernel on a second stream (TrainStep's arrangement)
            with defer_wgrad() as d:
                rgb = shade_posenc(net, pts, emb, ray_id, freq)
                rgb.backward(g_rgb)
            d.flush()
        else:
            rgb = shade_posenc(net, pts, emb, ray_id, freq)
            rgb.backward(g_rgb)
        PO.assert_close('rgb', rgb.detach(), ref['rgb'], mags['rgb'], PO.K_ROW)
        l1, l2, l3 = net[0], net[2][0], net[3]
        for k, p in zip(PO.SUM_KEYS, (l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias)):
            PO.assert_close(k, p.grad, ref[k], mags[k], PO.K_SUM)


def test_unsupported_shapes_fall_back_to_torch():
    from directvoxgo_amd.shade import shade_posenc, viewdir_embed
    pts = torch.rand((100, 3), device='cuda')
    emb = viewdir_embed(F.normalize(torch.randn((10, 3), device='cuda'), dim=-1), torch.tensor([1.0, 2.0, 4.0, 8.0], device='cuda'))
    rid = torch.randint(0, 10, (100,), device='cuda')
    assert shade_posenc(_head(12, 0), pts, emb, rid, torch.tensor([2.0 ** i for i in range(12)], device='cuda')) is None  # d_in 102
    from directvoxgo_amd.dvgo import make_rgbnet
    assert shade_posenc(make_rgbnet(3 + 6 * 4 + 27, 64, 3).cuda(), pts, emb, rid, torch.tensor([1.0, 2.0, 4.0, 8.0], device='cuda')) is None


@pytest.mark.parametrize('name', FIXTURES)
def test_positions_equal_sample_ray(name):
    """The positions the fused march hands the head are sample_ray's ray_pts of the same (ray, step) bit for bit, and
    the reference's own head input (positions first) too."""
    from directvoxgo_amd.fused import fused_march
    g = load_golden(name)
    m = build_model(g, True)
    ro, rd = cu(g['rays_o']), cu(g['rays_d'])
    rk = rk_of(g)
    cfg = m._march_cfg(rk['near'], rk['far'], rk['stepsize'])
    _, _, _, pts, ray_id, step_id, _ = fused_march(m.density, m.k0.detach()[:, :0], ro, rd, cfg, positions=True)
    sp, sr, ss = m.sample_ray(rays_o=ro, rays_d=rd, **rk)
    S = int(ss.max()) + 1
    lookup = torch.full((ro.shape[0] * S,), -1, dtype=torch.int64, device='cuda')
    lookup[sr * S + ss] = torch.arange(sr.shape[0], device='cuda')
    idx = lookup[ray_id * S + step_id]
    assert bool((idx >= 0).all())
    assert torch.equal(pts, sp[idx])
    assert np.array_equal(pts.cpu().numpy(), g['head_input'][:, :3])


@pytest.mark.parametrize('fused', [True, False])
def test_k0_is_never_read(fused):
    """k0 full of NaN: every output and gradient stays finite and equal to the run with the fixture's k0."""
    g = load_golden('forward_fine_posenc')
    outs = []
    for nan in (False, True):
        m = build_model(g, fused)
        if nan:
            with torch.no_grad():
                m.k0.fill_(float('nan'))
        res, loss = run(m, g)
        assert m.k0.grad is None
        outs.append((res, loss.detach(), m.density.grad, [p.grad for p in m.rgbnet.parameters()]))
    (a, la, da, ga), (b, lb, db, gb) = outs
    for k in a:
        assert torch.isfinite(b[k]).all() and torch.equal(a[k].detach(), b[k].detach()), k
    assert torch.equal(la, lb)
    assert torch.isfinite(db).all() and torch.allclose(da, db, rtol=1e-5, atol=1e-7)         # (atomic summation order)
    for x, y in zip(ga, gb):
        assert torch.isfinite(y).all() and torch.allclose(x, y, rtol=1e-5, atol=1e-7)


def _scene_model(sc, fused, P=10):
    from directvoxgo_amd.dvgo import DirectVoxGO
    w = sc['world']
    m = DirectVoxGO(sc['xyz_min'], sc['xyz_max'], num_voxels=w ** 3, num_voxels_base=w ** 3, alpha_init=1e-2,
                    fast_color_thres=1e-4, rgbnet_dim=12, rgbnet_width=128, rgbnet_direct=True, posbase_pe=P, fused=fused)
    torch.manual_seed(1)
    for p in m.rgbnet.parameters():
        torch.nn.init.normal_(p, std=0.1)
    m = m.cuda()
    with torch.no_grad():
        m.density.copy_(sc['density']); m.k0.copy_(sc['k0']); m.mask_cache.mask.copy_(sc['mask'])
    return m


def test_fused_equals_unfused_on_larger_scene():
    """The lego-like 160^3 scene (scenes.synthetic_scene): the fused march + HIP head against the op-by-op path with the
    torch head.  Index and march outputs are bit-exact (test_gpu_forward's argument); the head agrees to fp32 rounding."""
    from directvoxgo_amd.scenes import synthetic_scene
    sc = synthetic_scene(world=160, n_rays=4096, seed=5, device='cuda')
    outs = {}
    for fused in (True, False):
        m = _scene_model(sc, fused)
        res = m(sc['rays_o'], sc['rays_d'], sc['viewdirs'], near=sc['near'], far=sc['far'], bg=1, stepsize=0.5, render_depth=True)
        loss = loss_fn(res, sc['target'], 4096)
        loss.backward()
        assert m.k0.grad is None
        outs[fused] = (res, m.density.grad, [p.grad for p in m.rgbnet.parameters()])
    (a, da, ga), (b, db, gb) = outs[True], outs[False]
    assert a['ray_id'].shape[0] > 100000
    assert torch.equal(a['ray_id'], b['ray_id']) and torch.equal(a['weights'], b['weights'])
    assert torch.equal(a['raw_alpha'], b['raw_alpha']) and torch.equal(a['alphainv_last'], b['alphainv_last'])
    assert torch.allclose(a['raw_rgb'], b['raw_rgb'], rtol=1e-4, atol=1e-5)
    assert torch.allclose(a['rgb_marched'], b['rgb_marched'], atol=2e-5)
    assert torch.allclose(a['depth'], b['depth'], rtol=1e-4, atol=1e-2)
    for x, y in [(da, db)] + list(zip(ga, gb)):
        assert (x - y).abs().max() <= 1e-3 * y.abs().max() + 1e-7


def test_train_step_equals_the_manual_loop():
    """Three TrainStep steps against model(...); loss.backward(); optimizer.step() on a copy: same parameters; k0 bitwise
    unchanged and without optimizer state (MaskedAdam skips a parameter whose .grad is None, lib/masked_adam.py:48);
    the step is not capturable."""
    from directvoxgo_amd.scenes import synthetic_scene
    from directvoxgo_amd.train import FINE_TRAIN, TrainStep, create_optimizer_or_freeze_model, render_loss
    sc = synthetic_scene(world=64, n_rays=4096, seed=6, device='cuda')
    cfg = dict(FINE_TRAIN)
    rk = dict(near=sc['near'], far=sc['far'], bg=1, stepsize=0.5)
    ma, mb = _scene_model(sc, True), _scene_model(sc, True)
    k0_before = ma.k0.detach().clone()
    step = TrainStep(ma, cfg, rk)
    assert not step.can_capture()
    opt = create_optimizer_or_freeze_model(mb, cfg, global_step=0)
    decay = 0.1 ** (1 / (cfg['lrate_decay'] * 1000))
    args = (sc['rays_o'], sc['rays_d'], sc['viewdirs'], sc['target'])
    for s in (1, 2, 3):
        la = step(*args, global_step=s)
        res = mb(*args[:3], global_step=s, **rk)
        opt.zero_grad(set_to_none=True)
        lb = render_loss(res, sc['target'], 4096, cfg)
        lb.backward()
        assert mb.k0.grad is None
        opt.step()
        for grp in opt.param_groups:
            grp['lr'] = grp['lr'] * decay
        np.testing.assert_allclose(float(la), float(lb), rtol=1e-5)
    assert torch.equal(ma.k0.detach(), k0_before) and torch.equal(mb.k0.detach(), k0_before)
    assert ma.k0 not in step.optimizer.state and mb.k0 not in opt.state
    d = (ma.density.detach() - mb.density.detach()).abs()
    assert float((d > 1e-4).float().mean()) <= 1e-3 and float(d.max()) <= 0.35      # (atomic order: Adam noise, 3 x lr 0.1)
    for (k, p), q in zip(ma.rgbnet.named_parameters(), mb.rgbnet.parameters()):
        np.testing.assert_allclose(p.detach().cpu().numpy(), q.detach().cpu().numpy(), atol=5e-5, err_msg=k)


def test_mesh_colours_are_the_head_at_the_vertices():
    """extract_mesh(color=True) of a posenc model: the head evaluated by torch ops at the vertex positions, viewed along
    -normal (no k0 involved)."""
    from directvoxgo_amd.export import extract_mesh
    g = load_golden('forward_fine_posenc')
    m = build_model(g, True)
    mesh = extract_mesh(m, alpha_thres=0.5, color=True)
    v, nrm = mesh.vertices, mesh.normals
    assert v.shape[0] > 100
    with torch.no_grad():
        pe = (v.unsqueeze(-1) * m.posfreq).flatten(-2)
        pe = torch.cat([v, pe.sin(), pe.cos()], -1)
        d = -nrm
        ve = (d.unsqueeze(-1) * m.viewfreq).flatten(-2)
        ve = torch.cat([d, ve.sin(), ve.cos()], -1)
        ref = torch.sigmoid(m.rgbnet(torch.cat([pe, ve], -1)))
    assert torch.allclose(mesh.colors, ref, atol=2e-5)


def test_render_viewpoints_chunked_equals_single_pass():
    from directvoxgo_amd.render import get_rays_of_a_view, render_viewpoints
    from directvoxgo_amd.scenes import pose_spherical
    g = load_golden('forward_fine_posenc')
    m = build_model(g, True)
    H, W, focal = 128, 128, 200.0       # 16384 rays = 2 full chunks of 8192 + 1 empty chunk
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]], np.float32)
    pose = pose_spherical(30.0, -30.0, 3.0)
    rk = dict(near=0.5, far=6.0, bg=1, stepsize=0.5, inverse_y=False)
    rgbs, depths = render_viewpoints(m, [pose.numpy()], [(H, W)], [K], False, rk, chunk=8192)
    ro, rd, vd = get_rays_of_a_view(H, W, K, pose.cuda(), False, False, False, False)
    with torch.no_grad():
        res = m(ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous(), vd.reshape(-1, 3).contiguous(),
                render_depth=True, **rk)
    np.testing.assert_allclose(rgbs[0].reshape(-1, 3), res['rgb_marched'].cpu().numpy(), atol=1e-6)
    np.testing.assert_allclose(depths[0].reshape(-1), res['depth'].cpu().numpy(), atol=1e-4)
