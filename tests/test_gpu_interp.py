"""GPU: the bilinear plane decoder's kernels (csrc/plane_rows.hip) against the oracle of tests/interp_oracle.py, and
InterpTriPlaneVoxGO against the reference fixtures of tests/golden/make_golden_interp.py, fused against unfused, with
external planes, through the training step, a checkpoint and scale_volume_grid.

What is asked (u = 2^-24; A = the sum of the |terms| of a result), derived, not tuned:
  rows      the feat, q and cell columns are the oracle's float32 numbers bit for bit (the same operations in the same
            order; the oracle's fma is correctly rounded), and the feat columns are dvgo_triplane_fwd's 'concat' output bit
            for bit; a sin / cos column is within ENC_ULPS u |value| = 4 u |value| of the float64 sin / cos of the same
            float32 argument, what tests/posenc_oracle.py allows sinf / cosf of an exact argument;
  scatter   |got - exp| <= (n + 2) u A per texel with n contributions, the tri-plane scatter's bound (the same sum: each
            product w * g rounds once, n - 1 additions round once each on a partial sum of at most A); a texel with no
            contribution keeps its value.
"""
import copy
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden

import interp_oracle as IO
from test_gpu_triplane import cu, lay_out, loss_fn, rk_of

pytestmark = pytest.mark.gpu

AGGS = ('concat', 'sum')
MN, MX = np.array([-1.0, -0.8, -0.6], np.float32), np.array([0.9, 1.1, 0.7], np.float32)
SIZES = {'xy': (6, 7), 'yz': (3, 9), 'zx': (8, 1)}       # different, non-square, an axis of size 1
WS = (13, 1, 9)                                         # the tables: independent of the planes, an extent of 1
MS = (0, 1, 63, 64, 65, 1000)


def points(M, rng):
    """Up to 5 % outside the box; the box corners first, then texel centres of each plane and nodes of each table."""
    xyz = (rng.random((M, 3)) * (MX - MN) * 1.1 + MN - 0.05 * (MX - MN)).astype(np.float32)
    special = [[(MN, MX)[(i >> a) & 1][a] for a in range(3)] for i in range(8)]
    for key, (H, W) in SIZES.items():
        ah, aw = IO.TO.AXES[key]
        ia, ib = IO.TABLE[key]
        for hh, ww in ((H, W), (WS[ia], WS[ib])):
            for i in range(4):
                p = (MN + (MX - MN) * rng.random(3)).astype(np.float32)
                p[ah] = MN[ah] + (MX[ah] - MN[ah]) * np.float32((i % hh) / max(hh - 1, 1))
                p[aw] = MN[aw] + (MX[aw] - MN[aw]) * np.float32((i % ww) / max(ww - 1, 1))
                special.append(p)
    special = np.array(special, np.float32)[:M]
    xyz[:len(special)] = special
    return xyz


@functools.lru_cache(maxsize=None)
def rows_case(C, M, P, cell):
    """planes, points and the oracle's rows (float32 and float64) of one case: computed once, shared by the layouts"""
    rng = np.random.default_rng(100000 * C + 100 * M + 10 * P + int(cell))
    planes = {k: rng.standard_normal((1, C, *hw)).astype(np.float32) for k, hw in SIZES.items()}
    xyz = points(M, rng)
    r32 = IO.rows(planes, xyz, MN, MX, WS, P, cell)
    r64 = IO.rows(planes, xyz, MN, MX, WS, P, cell, np.float64)
    return planes, xyz, r32, r64


@pytest.mark.parametrize('layout', ['cf', 'cl', 'off'])
@pytest.mark.parametrize('C', [1, 3, 4, 32])
def test_rows_against_the_oracle(C, layout):
    from directvoxgo_amd.ops import plane_rows_fwd, triplane_fwd
    mn, mx = cu(MN), cu(MX)
    worst = 0.0
    for P in (1, 5):
        for cell in (True, False):
            cols, D = IO.columns(C, P, cell)
            for M in MS:
                planes, xyz, r32, r64 = rows_case(C, M, P, cell)
                dev = {k: lay_out(p, layout) for k, p in planes.items()}
                inp = plane_rows_fwd(dev, cu(xyz), mn, mx, WS, P, cell)
                assert inp.shape == r32.shape == (3, M, D), (M, P, cell)
                got = inp.cpu().numpy()
                for k in ('feat', 'q', 'cell'):
                    assert np.array_equal(got[..., cols[k]].view(np.uint32), r32[..., cols[k]].view(np.uint32)), (k, M, P, cell)
                tri = triplane_fwd(dev, cu(xyz), mn, mx, 'concat')
                assert torch.equal(inp[..., :C].permute(1, 0, 2).reshape(M, 3 * C), tri), (M, P, cell)
                for k in ('sin', 'cos'):
                    exp = r64[..., cols[k]]
                    err, bound = np.abs(got[..., cols[k]].astype(np.float64) - exp), IO.ENC_ULPS * IO.U * np.abs(exp)
                    if M:
                        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
                    assert (err <= bound).all(), (k, M, P, cell, float((err / np.maximum(bound, 1e-300)).max()))
    print(f'C={C} {layout}: worst sin / cos err / bound {worst:.3f}')


def test_rows_with_every_corner_outside():
    from directvoxgo_amd.ops import plane_rows_fwd
    planes = {k: np.ones((1, 4, *hw), np.float32) for k, hw in SIZES.items()}
    xyz = np.array([[5, -7, 9], [-1.8, 2.2, -1.8], [1e30, -1e30, 1e30]], np.float32)
    cols, D = IO.columns(4, 3, True)
    ws = (13, 4, 9)
    inp = plane_rows_fwd({k: cu(p) for k, p in planes.items()}, cu(xyz), cu(MN), cu(MX), ws, 3, True).cpu().numpy()
    assert (inp[..., cols['feat']] == 0).all() and (inp[..., cols['q']] == 0).all()
    assert (inp[..., cols['sin']] == 0).all() and (inp[..., cols['cos']] == 1).all()
    assert np.array_equal(inp[..., cols['cell']], IO.rows(planes, xyz, MN, MX, ws, 3, True)[..., cols['cell']])


@functools.lru_cache(maxsize=None)
def scatter_case(C, M, P, cell):
    rng = np.random.default_rng(200000 * C + 100 * M + 10 * P + int(cell))
    xyz = points(M, rng)
    D = IO.columns(C, P, cell)[1]
    ginp = rng.standard_normal((3, M, D)).astype(np.float32)
    ref = IO.scatter({k: (C, *hw) for k, hw in SIZES.items()}, xyz, MN, MX, ginp)
    return xyz, ginp, ref


@pytest.mark.parametrize('layout', ['cf', 'cl', 'off'])
@pytest.mark.parametrize('C', [1, 3, 4, 32])
def test_scatter_against_oracle(C, layout):
    from directvoxgo_amd.ops import plane_rows_bwd
    mn, mx = cu(MN), cu(MX)
    shapes = {k: (C, *hw) for k, hw in SIZES.items()}
    worst = 0.0
    for P, cell in ((1, False), (5, True)):
        for M in MS:
            xyz, ginp, ref = scatter_case(C, M, P, cell)
            for run in (0, 1, 8):
                grads = {k: lay_out(np.zeros((1, *s), np.float32), layout) for k, s in shapes.items()}
                plane_rows_bwd(cu(ginp), grads, cu(xyz), mn, mx, WS, P, cell, run=run)
                for k in IO.KEYS:
                    g, A, n = ref[k]
                    gg = grads[k][0].cpu().numpy().astype(np.float64)
                    err, bound = np.abs(gg - g), (n[None] + 2) * IO.U * A
                    assert (err <= bound).all(), (M, P, cell, run, k, float((err - bound).max()))
                    assert (gg[:, n == 0] == 0).all(), (M, P, cell, run, k)
                    if M:
                        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    print(f'C={C} {layout}: worst scatter err / bound {worst:.3f}')


def test_scatter_accumulates_and_never_reads_past_the_features():
    """Into non-zero caller buffers; with NaN in every column >= C of grad_inp the plane gradients are finite, within the
    same bound of the same sum, and equal bit for bit wherever the atomics' order cannot matter (at most one term)."""
    from directvoxgo_amd.ops import plane_rows_bwd
    rng = np.random.default_rng(7)
    C, M, P = 4, 200, 2
    xyz = points(M, rng)
    ginp = rng.standard_normal((3, M, C + 2 + 4 * P + 2)).astype(np.float32)
    start = {k: rng.standard_normal((1, C, *hw)).astype(np.float32) for k, hw in SIZES.items()}
    ref = IO.scatter({k: p.shape[1:] for k, p in start.items()}, xyz, MN, MX, ginp)
    poisoned = ginp.copy()
    poisoned[..., C:] = np.nan
    outs = []
    for g in (ginp, poisoned):
        grads = {k: lay_out(p, 'cl') for k, p in start.items()}
        plane_rows_bwd(cu(g), grads, cu(xyz), cu(MN), cu(MX), WS, P, True)
        outs.append({k: grads[k][0].cpu().numpy() for k in IO.KEYS})
    for k in IO.KEYS:
        g, A, n = ref[k]
        for got in (outs[0][k], outs[1][k]):
            assert np.isfinite(got).all()
            err = np.abs(got.astype(np.float64) - (g + start[k][0]))
            assert (err <= (n[None] + 3) * IO.U * (A + np.abs(start[k][0]))).all()         # one more term: the start value
            assert np.array_equal(got[:, n == 0], start[k][0][:, n == 0])
    # the atomics' order may differ between two launches; where a texel has at most one contribution it cannot
    for k in IO.KEYS:
        once = ref[k][2] <= 1
        assert np.array_equal(outs[0][k][:, once], outs[1][k][:, once])


# ---------------------------------------------------------------------------------------------- op and model
def _load(nets_owner, z, prefix):
    sd = {k[len(prefix):]: torch.from_numpy(v) for k, v in z.items() if k.startswith(prefix)}
    missing, unexpected = nets_owner.load_state_dict(sd, strict=False)
    assert not unexpected and not [k for k in missing if k.startswith(('interp_', 'rgbnet.'))]


@pytest.mark.parametrize('cell', [True, False])
@pytest.mark.parametrize('agg', AGGS)
def test_decode_reproduces_the_reference_fixture(agg, cell):
    """ops.interp_decode with the fixture's MLPs (float32, rocBLAS) on interp.npz at the LIIF fixture test's tolerances:
    values rtol 1e-4 / atol 1e-5, plane gradients rtol 1e-4 / atol 1e-6, MLP parameter gradients rtol 1e-3 / atol 1e-6; from
    channel-first planes (the samples outnumber the texels: channels-last copies) and from channels-last ones; no gradient
    for xyz or interp_zx."""
    from directvoxgo_amd.liif import InterpMLP
    from directvoxgo_amd.ops import interp_decode
    z = load_golden('interp')
    C, P = z['plane_xy'].shape[1], int(z['posbase_pe'])
    p = f'{agg}_c{int(cell)}_'
    for layout in ('cf', 'cl'):
        holder = torch.nn.Module()
        for net in ('interp_xy', 'interp_yz', 'interp_zx'):
            setattr(holder, net, InterpMLP(C + 2 + 4 * P + (2 if cell else 0), C, width=8, depth=3))
        _load(holder, z, f'c{int(cell)}_sd_')
        holder = holder.cuda().eval()
        planes = {k: lay_out(z['plane_' + k], layout).requires_grad_() for k in IO.KEYS}
        xyz = cu(z['xyz']).requires_grad_()
        out = interp_decode(planes, {'xy': holder.interp_xy, 'yz': holder.interp_yz}, xyz, cu(z['xyz_min']), cu(z['xyz_max']),
                            z['world_size'], P, cell, agg)
        err = np.abs(out.detach().cpu().numpy() - z[p + 'out'])
        print(f'{p}{layout}: worst value |err| {err.max():.3g}')
        np.testing.assert_allclose(out.detach().cpu().numpy(), z[p + 'out'], rtol=1e-4, atol=1e-5)
        out.backward(cu(z[agg + '_gout']))
        assert xyz.grad is None
        for k in IO.KEYS:
            assert planes[k].grad.shape == planes[k].shape
            np.testing.assert_allclose(planes[k].grad.cpu().numpy(), z[f'{p}gplane_{k}'], rtol=1e-4, atol=1e-6)
        for name, q in holder.named_parameters():
            if name.startswith('interp_zx.'):
                assert q.grad is None
            else:
                np.testing.assert_allclose(q.grad.cpu().numpy(), z[f'{p}g_{name}'], rtol=1e-3, atol=1e-6)


def build_model(g, z, fused):
    from directvoxgo_amd.interp import InterpTriPlaneVoxGO
    nv = int(np.prod(g['world_size']))
    m = InterpTriPlaneVoxGO(g['xyz_min'], g['xyz_max'], num_voxels=nv, num_voxels_base=nv, alpha_init=1e-2,
                            fast_color_thres=float(g['fast_color_thres']), fused=fused, rgbnet_dim=int(g['rgbnet_dim']),
                            rgbnet_depth=3, rgbnet_width=64, viewbase_pe=4, rgbnet_direct=False, implicit_voxel_feat=True,
                            liif=False, cell_decode=True, interp_width=16, interp_depth=3, tri_aggregation='sum', posbase_pe=2,
                            cat_posemb=True)
    assert tuple(int(v) for v in m.world_size) == tuple(g['world_size'])
    with torch.no_grad():
        m.density.copy_(torch.from_numpy(g['density']))
        m.mask_cache.mask.copy_(torch.from_numpy(g['mask']))
    _load(m, z, 'sd_')
    return m.cuda().eval()                                   # eval(): the fixture was made with dropout off


@pytest.mark.parametrize('fused', [True, False])
def test_forward_matches_reference_orchestration(fused):
    """forward_interp.npz at the tolerances of test_gpu_liif.test_forward_matches_reference_orchestration for the same
    quantities; the planes are the caller's (render(feats=...)): the gradients arrive there and model.planes stays without
    one; interp_zx gets none."""
    g, z = load_golden('forward_triplane'), load_golden('forward_interp')
    m = build_model(g, z, fused)
    feats = {k: cu(g['plane_' + k]).requires_grad_() for k in IO.KEYS}
    ro, rd, vd = cu(g['rays_o']), cu(g['rays_d']), cu(g['viewdirs'])
    res = m.render(feats, ro, rd, vd, 0, **rk_of(g))
    loss = loss_fn(res, cu(g['target']), ro.shape[0])
    loss.backward()
    assert np.array_equal(res['ray_id'].cpu().numpy(), z['out_ray_id'])
    np.testing.assert_allclose(res['weights'].detach().cpu().numpy(), z['out_weights'], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(res['raw_alpha'].detach().cpu().numpy(), z['out_raw_alpha'], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(res['alphainv_last'].detach().cpu().numpy(), z['out_alphainv_last'], rtol=1e-5, atol=1e-6)
    print('worst raw_rgb |err|', float(np.abs(res['raw_rgb'].detach().cpu().numpy() - z['out_raw_rgb']).max()))
    np.testing.assert_allclose(res['raw_rgb'].detach().cpu().numpy(), z['out_raw_rgb'], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(res['rgb_marched'].detach().cpu().numpy(), z['out_rgb_marched'], atol=1e-5)
    np.testing.assert_allclose(res['depth'].cpu().numpy(), z['out_depth'], rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(float(loss), float(z['loss']), rtol=1e-5)
    np.testing.assert_allclose(m.density.grad.cpu().numpy(), z['grad_density'], rtol=1e-4, atol=1e-6)
    for k in IO.KEYS:
        np.testing.assert_allclose(feats[k].grad.cpu().numpy(), z[f'grad_plane_{k}'], rtol=1e-4, atol=1e-6)
        assert m.planes[k].grad is None
    for k, q in m.named_parameters():
        if k.startswith(('rgbnet.', 'interp_xy.', 'interp_yz.')):
            np.testing.assert_allclose(q.grad.cpu().numpy(), z[f'grad_{k}'], rtol=1e-3, atol=1e-6, err_msg=k)
        elif k.startswith('interp_zx.'):
            assert q.grad is None


def test_fused_equals_unfused():
    """Both paths decode at bit-equal positions with the same kernels and the same GEMM shapes: with torch's colour head
    behind them every per-sample and per-ray output is equal, rgb_marched included."""
    g, z = load_golden('forward_triplane'), load_golden('forward_interp')
    ro, rd, vd = cu(g['rays_o']), cu(g['rays_d']), cu(g['viewdirs'])
    planes = {k: cu(g['plane_' + k]) for k in IO.KEYS}
    outs = {}
    for fused in (True, False):
        m = build_model(g, z, fused)
        m.fused_shade = False
        with torch.no_grad():
            outs[fused] = m.render(planes, ro, rd, vd, **rk_of(g))
    a, b = outs[True], outs[False]
    assert a['ray_id'].shape[0] > 100
    for k in ('ray_id', 'weights', 'raw_alpha', 'alphainv_last', 'raw_rgb', 'rgb_marched', 'depth'):
        assert torch.equal(a[k], b[k]), k


def test_a_batch_that_keeps_no_sample():
    """A chunk of background rays, or one that fast_color_thres filters entirely: interp_decode on no position gives the
    empty result of the right width (and zero plane gradients), and render on rays that miss the box gives empty per-sample
    outputs and rgb_marched == bg, on the fused and the op-by-op path."""
    from directvoxgo_amd.liif import InterpMLP
    from directvoxgo_amd.ops import interp_decode
    C, P = 4, 2
    nets = {k: InterpMLP(C + 2 + 4 * P + 2, C, width=8, depth=3).cuda().eval() for k in ('xy', 'yz')}
    for agg in AGGS:
        planes = {k: cu(np.ones((1, C, *hw), np.float32)).requires_grad_() for k, hw in SIZES.items()}
        out = interp_decode(planes, nets, torch.zeros(0, 3, device='cuda'), cu(MN), cu(MX), WS, P, True, agg)
        assert out.shape == (0, 3 * C if agg == 'concat' else C)
        out.sum().backward()
        assert all(q.grad is None or not q.grad.any() for q in planes.values())
    g, z = load_golden('forward_triplane'), load_golden('forward_interp')
    N = 37
    ro = cu(np.tile(g['xyz_max'] + 3, (N, 1)).astype(np.float32))
    rd = cu(np.tile(np.float32([1, 0.1, 0.1]), (N, 1)))                     # away from the box
    vd = rd / rd.norm(dim=-1, keepdim=True)
    planes = {k: cu(g['plane_' + k]) for k in IO.KEYS}
    rk = rk_of(g)
    for fused in (True, False):
        m = build_model(g, z, fused)
        with torch.no_grad():
            res = m.render(planes, ro, rd, vd, **rk)
        assert res['ray_id'].shape == (0,) and res['weights'].shape == (0,) and res['raw_alpha'].shape == (0,), fused
        assert res['raw_rgb'].shape == (0, 3) and res['depth'].shape == (N,), fused
        assert torch.equal(res['alphainv_last'], torch.ones(N, device='cuda')), fused
        assert torch.equal(res['rgb_marched'], torch.full((N, 3), float(rk['bg']), device='cuda')), fused


def test_train_step_checkpoint_and_scale_volume_grid(tmp_path):
    """TrainStep on scenes.synthetic_scene: the first step lowers the loss of its batch, the steps move planes, density,
    rgbnet, interp_xy and interp_yz and leave interp_zx where it was (no gradient ever reaches it); a checkpoint written
    after them and loaded into a fresh model gives the same state and kwargs; after scale_volume_grid the rows are the
    oracle's at the new world_size (feat, q, cell bit for bit), and the decoder agrees with the float64 oracle at an MLP
    output's tolerance (rtol 1e-4 / atol 1e-5)."""
    from directvoxgo_amd.checkpoint import load_checkpoint, load_model, save_checkpoint
    from directvoxgo_amd.interp import TRI_INTERP_FINE_TRAIN, InterpTriPlaneVoxGO
    from directvoxgo_amd.ops import plane_rows_fwd
    from directvoxgo_amd.scenes import synthetic_scene
    from directvoxgo_amd.train import TrainStep, create_optimizer_or_freeze_model
    sc = synthetic_scene(world=32, n_rays=2048, seed=6, device='cuda')
    cfg = dict(TRI_INTERP_FINE_TRAIN)
    rk = dict(near=sc['near'], far=sc['far'], bg=1, stepsize=0.5)
    m = InterpTriPlaneVoxGO(sc['xyz_min'], sc['xyz_max'], num_voxels=32 ** 3, num_voxels_base=32 ** 3, alpha_init=1e-2,
                            fast_color_thres=1e-4, rgbnet_dim=4, rgbnet_width=64, tri_aggregation='sum', interp_width=16,
                            interp_depth=3, interp_dropout=0.0, posbase_pe=3, cat_posemb=True)
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
    assert all(np.isfinite(losses)) and losses[1] < losses[0]
    after = m.state_dict()
    for k in ('density', 'planes.xy', 'planes.yz', 'planes.zx', 'rgbnet.0.weight', 'interp_xy.model.0.weight',
              'interp_xy.model.3.bias', 'interp_yz.model.0.weight', 'interp_yz.model.2.0.weight'):
        assert not torch.equal(before[k], after[k]), k
    for k in after:
        if k.startswith('interp_zx.'):
            assert torch.equal(before[k], after[k]), k
    path = str(tmp_path / 'interp.tar')
    save_checkpoint(path, m, step.optimizer, 3)
    m2 = load_model(InterpTriPlaneVoxGO, path).cuda()
    assert m2.get_kwargs().keys() == m.get_kwargs().keys() and m2.cell_decode and m2.cat_posemb and m2.posbase_pe == 3
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
    cols, D = IO.columns(4, 3, True)
    inp = plane_rows_fwd(m.planes, cu(xyz), m.xyz_min, m.xyz_max, ws, m.posbase_pe, m.cell_decode).cpu().numpy()
    e32 = IO.rows(host, xyz, mn, mx, ws, 3, True)
    e64 = IO.rows(host, xyz, mn, mx, ws, 3, True, np.float64)
    for k in ('feat', 'q', 'cell'):
        assert np.array_equal(inp[..., cols[k]], e32[..., cols[k]]), k
    for k in ('sin', 'cos'):
        assert (np.abs(inp[..., cols[k]] - e64[..., cols[k]]) <= IO.ENC_ULPS * IO.U * np.abs(e64[..., cols[k]])).all(), k
    with torch.no_grad():
        got = m.sample_planes(cu(xyz)).cpu().numpy()
        nets = {k: copy.deepcopy(getattr(m, 'interp_' + k)).cpu().double().eval() for k in ('xy', 'yz')}
        exp = IO.decode({k: torch.from_numpy(v) for k, v in host.items()}, nets, xyz, mn, mx, ws, 3, True, 'sum').numpy()
    np.testing.assert_allclose(got, exp, rtol=1e-4, atol=1e-5)
