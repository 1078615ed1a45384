"""GPU: the LIIF plane decoder's kernels (csrc/liif.hip) against the oracle of tests/liif_oracle.py, and LIIFTriPlaneVoxGO
against the reference fixtures of tests/golden/make_golden_liif.py, fused against unfused, with external planes, through
the training step, a checkpoint and scale_volume_grid.

What is asked (u = 2^-24; A = the sum of the |terms| of a result), derived, not tuned:
  gather    inp and wgt are the oracle's float32 numbers bit for bit: the same operations in the same order, no sum;
  scatter   |got - exp| <= (n + 2) u A per texel with n contributions, for any order of the atomics and of a lane's own
            run sums: the terms are the float32 inputs themselves (no product), and n - 1 additions (n with a non-zero
            start value) round once each on a partial sum of at most A; a texel with no contribution keeps its value;
  blend     forward |got - exp| <= (T + 1) u A: the weights are the oracle's float32 numbers, each of the T fused
            multiply-adds of a chain rounds once (T = E per plane; 'sum' adds the three chains: T = 3E covers its 3E + 2
            roundings' first-order bound of (E + 2) u A as well); backward is one float32 product: bit-equal.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden

import liif_oracle as LO
from test_gpu_triplane import cu, lay_out, loss_fn, rk_of

pytestmark = pytest.mark.gpu

AGGS = ('concat', 'sum')
MN, MX = np.array([-1.0, -0.8, -0.6], np.float32), np.array([0.9, 1.1, 0.7], np.float32)
# plane sizes and the world_size they are decoded against: different, non-square; an axis of size 1, a world extent of 2
GEOS = (({'xy': (6, 7), 'yz': (3, 9), 'zx': (8, 2)}, (13, 13, 9)),
        ({'xy': (1, 5), 'yz': (33, 4), 'zx': (2, 2)}, (2, 5, 7)))
MS = (0, 1, 63, 64, 65, 1000)


def points(M, rng):
    """Up to 5 % outside the box; the box corners and the centre first."""
    xyz = (rng.random((M, 3)) * (MX - MN) * 1.1 + MN - 0.05 * (MX - MN)).astype(np.float32)
    special = [[(MN, MX)[(i >> a) & 1][a] for a in range(3)] for i in range(8)] + [(MN + MX) / 2]
    special = np.array(special, np.float32)[:M]
    xyz[:len(special)] = special
    return xyz


@pytest.mark.parametrize('layout', ['cf', 'cl', 'off'])
@pytest.mark.parametrize('C', [1, 3, 4, 32])
def test_gather_is_the_oracle_bit_for_bit(C, layout):
    from directvoxgo_amd.ops import liif_gather_fwd
    rng = np.random.default_rng(2000 * C + len(layout))
    mn, mx = cu(MN), cu(MX)
    for sizes, ws in GEOS:
        planes = {k: rng.standard_normal((1, C, *hw)).astype(np.float32) for k, hw in sizes.items()}
        dev = {k: lay_out(p, layout) for k, p in planes.items()}
        for M in MS:
            xyz = points(M, rng)
            for cell in (True, False):
                for ens in (True, False):
                    inp, wgt = liif_gather_fwd(dev, cu(xyz), mn, mx, ws, cell, ens)
                    e_inp, e_wgt = LO.rows(planes, xyz, MN, MX, ws, cell, ens)
                    assert inp.shape == e_inp.shape == (3, 4 if ens else 1, M, C + (4 if cell else 2))
                    assert wgt.shape == e_wgt.shape
                    got_i, got_w = inp.cpu().numpy(), wgt.cpu().numpy()
                    assert np.array_equal(got_i.view(np.uint32), e_inp.view(np.uint32)), (sizes, M, cell, ens)
                    assert np.array_equal(got_w.view(np.uint32), e_wgt.view(np.uint32)), (sizes, M, cell, ens)


def test_gather_rounds_half_to_even():
    """Symmetric box, one position per sample (E = 1), plane rows of 6: the point at coordinate 0 has the unnormalised
    row index ((0 + 1) * 6 - 1) / 2 = 2.5, and 1/3 has 3.5: rint gives 2 and 4."""
    from directvoxgo_amd.ops import liif_gather_fwd
    one = np.ones(3, np.float32)
    rows = np.arange(6, dtype=np.float32)[None, None, :, None].repeat(5, 3)            # value = row index
    planes = {k: rows.copy() for k in LO.KEYS}
    xyz = np.array([[0, 0, 0], [1 / 3, 1 / 3, 1 / 3]], np.float32)
    inp, _ = liif_gather_fwd({k: cu(p) for k, p in planes.items()}, cu(xyz), cu(-one), cu(one), (6, 6, 6), False, False)
    assert inp.shape == (3, 1, 2, 3)
    assert inp[:, 0, :, 0].cpu().tolist() == [[2.0, 4.0]] * 3
    assert np.array_equal(inp.cpu().numpy(), LO.rows(planes, xyz, -one, one, (6, 6, 6), False, False)[0])


@pytest.mark.parametrize('layout', ['cf', 'cl', 'off'])
@pytest.mark.parametrize('C', [1, 3, 4, 32])
def test_scatter_against_oracle(C, layout):
    from directvoxgo_amd.ops import liif_gather_bwd
    rng = np.random.default_rng(3000 * C + len(layout))
    mn, mx = cu(MN), cu(MX)
    worst = 0.0
    for (sizes, ws), cell in zip(GEOS, (True, False)):
        shapes = {k: (C, *hw) for k, hw in sizes.items()}
        for M in MS:
            xyz = points(M, rng)
            for ens in (True, False):
                ginp = rng.standard_normal((3, 4 if ens else 1, M, C + (4 if cell else 2))).astype(np.float32)
                ref = LO.scatter(shapes, xyz, MN, MX, ws, ginp, ens)
                for run in (0, 1, 8):
                    grads = {k: lay_out(np.zeros((1, *s), np.float32), layout) for k, s in shapes.items()}
                    liif_gather_bwd(cu(ginp), grads, cu(xyz), mn, mx, ws, cell, ens, run=run)
                    for k in LO.KEYS:
                        g, A, n = ref[k]
                        gg = grads[k][0].cpu().numpy().astype(np.float64)
                        err, bound = np.abs(gg - g), (n[None] + 2) * LO.U * A
                        assert (err <= bound).all(), (sizes, M, ens, run, k, float((err - bound).max()))
                        assert (gg[:, n == 0] == 0).all(), (sizes, M, ens, run, k)
                        if M:
                            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    print(f'C={C} {layout}: worst scatter err / bound {worst:.3f}')


def test_scatter_accumulates_into_the_callers_buffers():
    from directvoxgo_amd.ops import liif_gather_bwd
    rng = np.random.default_rng(7)
    (sizes, ws), C, M = GEOS[0], 4, 200
    xyz = points(M, rng)
    ginp = rng.standard_normal((3, 4, M, C + 4)).astype(np.float32)
    start = {k: rng.standard_normal((1, C, *hw)).astype(np.float32) for k, hw in sizes.items()}
    grads = {k: lay_out(p, 'cl') for k, p in start.items()}
    liif_gather_bwd(cu(ginp), grads, cu(xyz), cu(MN), cu(MX), ws, True, True)
    ref = LO.scatter({k: p.shape[1:] for k, p in start.items()}, xyz, MN, MX, ws, ginp, True)
    for k in LO.KEYS:
        g, A, n = ref[k]
        got = grads[k][0].cpu().numpy()
        err = np.abs(got.astype(np.float64) - (g + start[k][0]))
        assert (err <= (n[None] + 3) * LO.U * (A + np.abs(start[k][0]))).all()         # one more term: the start value
        assert np.array_equal(got[:, n == 0], start[k][0][:, n == 0])


@pytest.mark.parametrize('C', [1, 3, 4, 32])
def test_blend_against_oracle(C):
    from directvoxgo_amd.ops import liif_blend_bwd, liif_blend_fwd
    rng = np.random.default_rng(4000 + C)
    worst = 0.0
    for M in MS:
        for E in (4, 1):
            pred = rng.standard_normal((3, E, M, C)).astype(np.float32)
            wgt = rng.random((3, E, M)).astype(np.float32)
            for agg in AGGS:
                T = E if agg == 'concat' else 3 * E
                got = liif_blend_fwd(cu(pred), cu(wgt), agg).cpu().numpy().astype(np.float64)
                exp, A = LO.blend(pred, wgt, agg)
                assert got.shape == exp.shape == (M, 3 * C if agg == 'concat' else C)
                err, bound = np.abs(got - exp), (T + 1) * LO.U * A
                assert (err <= bound).all(), (M, E, agg, float((err - bound).max()))
                if M:
                    worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
                gout = rng.standard_normal(exp.shape).astype(np.float32)
                gp = liif_blend_bwd(cu(gout), cu(wgt), C, agg).cpu().numpy()
                g = gout.reshape(M, 3, C).transpose(1, 0, 2) if agg == 'concat' else np.broadcast_to(gout, (3, M, C))
                e_gp = g[:, None] * wgt[..., None]
                assert e_gp.dtype == np.float32 and np.array_equal(gp.view(np.uint32), e_gp.view(np.uint32)), (M, E, agg)
    print(f'C={C}: worst blend err / bound {worst:.3f}')


# ---------------------------------------------------------------------------------------------- op and model
def _load(nets_owner, z, prefix):
    sd = {k[len(prefix):]: torch.from_numpy(v) for k, v in z.items() if k.startswith(prefix)}
    missing, unexpected = nets_owner.load_state_dict(sd, strict=False)
    assert not unexpected and not [k for k in missing if k.startswith(('interp_', 'rgbnet.'))]


@pytest.mark.parametrize('ens', [True, False])
@pytest.mark.parametrize('cell', [True, False])
@pytest.mark.parametrize('agg', AGGS)
def test_decode_reproduces_the_reference_fixture(agg, cell, ens):
    """ops.liif_decode with the fixture's MLPs (float32, rocBLAS) on liif.npz at the tolerances tests/test_gpu_triplane.py
    holds the same kinds of quantity to on forward_triplane.npz: an MLP's output (there raw_rgb) rtol 1e-4 / atol 1e-5,
    plane gradients rtol 1e-4 / atol 1e-6, MLP parameter gradients rtol 1e-3 / atol 1e-6; from channel-first planes (the
    samples outnumber the texels: channels-last copies) and from channels-last ones; no gradient for xyz or interp_zx."""
    from directvoxgo_amd.liif import InterpMLP
    from directvoxgo_amd.ops import liif_decode
    z = load_golden('liif')
    C = z['plane_xy'].shape[1]
    p = f'{agg}_c{int(cell)}_e{int(ens)}_'
    for layout in ('cf', 'cl'):
        holder = torch.nn.Module()
        for net in ('interp_xy', 'interp_yz', 'interp_zx'):
            setattr(holder, net, InterpMLP(C + (4 if cell else 2), C, width=8, depth=3))
        _load(holder, z, f'c{int(cell)}_sd_')
        holder = holder.cuda().eval()
        planes = {k: lay_out(z['plane_' + k], layout).requires_grad_() for k in LO.KEYS}
        xyz = cu(z['xyz']).requires_grad_()
        out = liif_decode(planes, {'xy': holder.interp_xy, 'yz': holder.interp_yz}, xyz, cu(z['xyz_min']), cu(z['xyz_max']),
                          z['world_size'], cell, ens, agg)
        err = np.abs(out.detach().cpu().numpy() - z[p + 'out'])
        print(f'{p}{layout}: worst value |err| {err.max():.3g}')
        np.testing.assert_allclose(out.detach().cpu().numpy(), z[p + 'out'], rtol=1e-4, atol=1e-5)
        out.backward(cu(z[agg + '_gout']))
        assert xyz.grad is None
        for k in LO.KEYS:
            assert planes[k].grad.shape == planes[k].shape
            np.testing.assert_allclose(planes[k].grad.cpu().numpy(), z[f'{p}gplane_{k}'], rtol=1e-4, atol=1e-6)
        for name, q in holder.named_parameters():
            if name.startswith('interp_zx.'):
                assert q.grad is None
            else:
                np.testing.assert_allclose(q.grad.cpu().numpy(), z[f'{p}g_{name}'], rtol=1e-3, atol=1e-6)


CASES = {'sum': dict(tri_aggregation='sum'), 'pe': dict(tri_aggregation='concat', posbase_pe=2, cat_posemb=True)}


def build_model(g, z, tag, fused):
    from directvoxgo_amd.liif import LIIFTriPlaneVoxGO
    nv = int(np.prod(g['world_size']))
    m = LIIFTriPlaneVoxGO(g['xyz_min'], g['xyz_max'], num_voxels=nv, num_voxels_base=nv, alpha_init=1e-2,
                          fast_color_thres=float(g['fast_color_thres']), fused=fused, rgbnet_dim=int(g['rgbnet_dim']),
                          rgbnet_depth=3, rgbnet_width=64, viewbase_pe=4, rgbnet_direct=False, implicit_voxel_feat=True,
                          liif=True, cell_decode=True, local_ensemble=True, interp_width=16, interp_depth=3, **CASES[tag])
    assert tuple(int(v) for v in m.world_size) == tuple(g['world_size'])
    with torch.no_grad():
        m.density.copy_(torch.from_numpy(g['density']))
        m.mask_cache.mask.copy_(torch.from_numpy(g['mask']))
    _load(m, z, tag + '_sd_')
    return m.cuda().eval()                                   # eval(): the fixture was made with dropout off


@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('tag', list(CASES))
def test_forward_matches_reference_orchestration(tag, fused):
    """forward_liif.npz at the tolerances of test_gpu_triplane.test_forward_matches_reference_orchestration for the same
    quantities, the Interp_MLPs' gradients at rgbnet's; the planes are the caller's (render(feats=...)): the gradients
    arrive there and model.planes stays without one; interp_zx gets none."""
    g, z = load_golden('forward_triplane'), load_golden('forward_liif')
    m = build_model(g, z, tag, fused)
    feats = {k: cu(g['plane_' + k]).requires_grad_() for k in LO.KEYS}
    ro, rd, vd = cu(g['rays_o']), cu(g['rays_d']), cu(g['viewdirs'])
    res = m.render(feats, ro, rd, vd, 0, **rk_of(g))
    loss = loss_fn(res, cu(g['target']), ro.shape[0])
    loss.backward()
    p = tag + '_'
    assert np.array_equal(res['ray_id'].cpu().numpy(), z[p + 'out_ray_id'])
    np.testing.assert_allclose(res['weights'].detach().cpu().numpy(), z[p + 'out_weights'], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(res['raw_alpha'].detach().cpu().numpy(), z[p + 'out_raw_alpha'], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(res['alphainv_last'].detach().cpu().numpy(), z[p + 'out_alphainv_last'], rtol=1e-5, atol=1e-6)
    print('worst raw_rgb |err|', float(np.abs(res['raw_rgb'].detach().cpu().numpy() - z[p + 'out_raw_rgb']).max()))
    np.testing.assert_allclose(res['raw_rgb'].detach().cpu().numpy(), z[p + 'out_raw_rgb'], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(res['rgb_marched'].detach().cpu().numpy(), z[p + 'out_rgb_marched'], atol=1e-5)
    np.testing.assert_allclose(res['depth'].cpu().numpy(), z[p + 'out_depth'], rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(float(loss), float(z[p + 'loss']), rtol=1e-5)
    np.testing.assert_allclose(m.density.grad.cpu().numpy(), z[p + 'grad_density'], rtol=1e-4, atol=1e-6)
    for k in LO.KEYS:
        np.testing.assert_allclose(feats[k].grad.cpu().numpy(), z[f'{p}grad_plane_{k}'], rtol=1e-4, atol=1e-6)
        assert m.planes[k].grad is None
    for k, q in m.named_parameters():
        if k.startswith(('rgbnet.', 'interp_xy.', 'interp_yz.')):
            np.testing.assert_allclose(q.grad.cpu().numpy(), z[f'{p}grad_{k}'], rtol=1e-3, atol=1e-6, err_msg=k)
        elif k.startswith('interp_zx.'):
            assert q.grad is None


@pytest.mark.parametrize('tag', list(CASES))
def test_fused_equals_unfused(tag):
    """Both paths decode at bit-equal positions with the same kernels and the same GEMM shapes: with torch's colour head
    behind them every per-sample and per-ray output is equal, rgb_marched included."""
    g, z = load_golden('forward_triplane'), load_golden('forward_liif')
    ro, rd, vd = cu(g['rays_o']), cu(g['rays_d']), cu(g['viewdirs'])
    planes = {k: cu(g['plane_' + k]) for k in LO.KEYS}
    outs = {}
    for fused in (True, False):
        m = build_model(g, z, tag, fused)
        m.fused_shade = False
        with torch.no_grad():
            outs[fused] = m.render(planes, ro, rd, vd, **rk_of(g))
    a, b = outs[True], outs[False]
    assert a['ray_id'].shape[0] > 100
    for k in ('ray_id', 'weights', 'raw_alpha', 'alphainv_last', 'raw_rgb', 'rgb_marched', 'depth'):
        assert torch.equal(a[k], b[k]), k


def test_train_step_checkpoint_and_scale_volume_grid(tmp_path):
    """Three TrainStep steps on scenes.synthetic_scene move planes, density, rgbnet, interp_xy and interp_yz and leave
    interp_zx where it was (no gradient ever reaches it); a checkpoint written after them and loaded into a fresh model
    gives the same state and kwargs; after scale_volume_grid the gather is the oracle's at the new world_size, bit for bit,
    and the decoder agrees with the float64 oracle at an MLP output's tolerance (rtol 1e-4 / atol 1e-5)."""
    from directvoxgo_amd.checkpoint import load_checkpoint, load_model, save_checkpoint
    from directvoxgo_amd.liif import TRI_LIIF_FINE_TRAIN, LIIFTriPlaneVoxGO
    from directvoxgo_amd.ops import liif_gather_fwd
    from directvoxgo_amd.scenes import synthetic_scene
    from directvoxgo_amd.train import TrainStep, create_optimizer_or_freeze_model
    sc = synthetic_scene(world=32, n_rays=2048, seed=6, device='cuda')
    cfg = dict(TRI_LIIF_FINE_TRAIN)
    rk = dict(near=sc['near'], far=sc['far'], bg=1, stepsize=0.5)
    m = LIIFTriPlaneVoxGO(sc['xyz_min'], sc['xyz_max'], num_voxels=32 ** 3, num_voxels_base=32 ** 3, alpha_init=1e-2,
                          fast_color_thres=1e-4, rgbnet_dim=4, rgbnet_width=64, tri_aggregation='sum', interp_width=16,
                          interp_depth=3)
    torch.manual_seed(1)
    for q in list(m.rgbnet.parameters()) + list(m.planes.values()):
        torch.nn.init.normal_(q, std=0.1)
    m = m.cuda()
    with torch.no_grad():
        m.density.copy_(sc['density']); m.mask_cache.mask.copy_(sc['mask'])
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    step = TrainStep(m, cfg, rk)
    assert not step.can_capture()
    args = (sc['rays_o'], sc['rays_d'], sc['viewdirs'], sc['target'])
    losses = [float(step(*args, global_step=s)) for s in (1, 2, 3)]
    print('losses', losses)
    assert all(np.isfinite(losses))
    after = m.state_dict()
    for k in ('density', 'planes.xy', 'planes.yz', 'planes.zx', 'rgbnet.0.weight', 'interp_xy.model.0.weight',
              'interp_xy.model.3.bias', 'interp_yz.model.0.weight', 'interp_yz.model.2.0.weight'):
        assert not torch.equal(before[k], after[k]), k
    for k in after:
        if k.startswith('interp_zx.'):
            assert torch.equal(before[k], after[k]), k
    path = str(tmp_path / 'liif.tar')
    save_checkpoint(path, m, step.optimizer, 3)
    m2 = load_model(LIIFTriPlaneVoxGO, path).cuda()
    assert m2.get_kwargs().keys() == m.get_kwargs().keys() and m2.cell_decode and m2.local_ensemble
    assert all(torch.equal(v, m2.state_dict()[k]) for k, v in m.state_dict().items())
    opt2 = create_optimizer_or_freeze_model(m2, cfg, global_step=0)
    _, opt2, gs = load_checkpoint(m2, opt2, path)
    assert gs == 3
    m.eval(); m2.eval()
    with torch.no_grad():
        ra, rb = m(*args[:3], **rk), m2(*args[:3], **rk)
    assert torch.equal(ra['rgb_marched'], rb['rgb_marched'])

    m.scale_volume_grid(40 ** 3)
    ws = tuple(int(v) for v in m.world_size)
    assert min(ws) > 32
    rng = np.random.default_rng(11)
    mn, mx = m.xyz_min.cpu().numpy(), m.xyz_max.cpu().numpy()
    xyz = (mn + (mx - mn) * rng.random((500, 3))).astype(np.float32)
    host = {k: q.detach().cpu().numpy() for k, q in m.planes.items()}
    inp, wgt = liif_gather_fwd(m.planes, cu(xyz), m.xyz_min, m.xyz_max, ws, m.cell_decode, m.local_ensemble)
    e_inp, e_wgt = LO.rows(host, xyz, mn, mx, ws, True, True)
    assert np.array_equal(inp.cpu().numpy(), e_inp) and np.array_equal(wgt.cpu().numpy(), e_wgt)
    with torch.no_grad():
        got = m.sample_planes(cu(xyz)).cpu().numpy()
        import copy
        nets = {k: copy.deepcopy(getattr(m, 'interp_' + k)).cpu().double().eval() for k in ('xy', 'yz')}
        exp = LO.decode({k: torch.from_numpy(v) for k, v in host.items()}, nets, xyz, mn, mx, ws, True, True, 'sum').numpy()
    np.testing.assert_allclose(got, exp, rtol=1e-4, atol=1e-5)
