"""GPU: SSIM / PSNR of csrc/metrics.hip against the reference's own numbers (tests/golden/metrics.npz) and the metrics
oracle (tests/metrics_oracle.c) at 800x800; bitwise reproducibility, alone vs in a batch; render_viewpoints /
evaluate_viewpoints with ground truth, in one process and over two gloo ranks."""
import os

import numpy as np
import pytest
import torch

import metrics_oracle as MO
from conftest import load_golden

pytestmark = pytest.mark.gpu

SSIM_TOL, MAP_TOL, PSNR_TOL = 1e-6, 1e-5, 1e-4


def _psnr_ok(p, ref):
    return p == ref if np.isinf(ref) else abs(p - ref) <= PSNR_TOL


def test_hip_metrics_match_the_reference_fixture():
    from directvoxgo_amd import metrics
    g = load_golden('metrics')
    for n in (str(x) for x in g['names']):
        max_val, fs, sigma = g[n + '/params']
        a, b = g[n + '/img0'], g[n + '/img1']
        s = metrics.ssim(a, b, max_val, filter_size=int(fs), filter_sigma=sigma)
        m = metrics.ssim(a, b, max_val, filter_size=int(fs), filter_sigma=sigma, return_map=True)
        p = metrics.psnr(a, b)
        assert abs(s - g[n + '/ssim']) <= SSIM_TOL, (n, s, g[n + '/ssim'])
        np.testing.assert_allclose(m.cpu().numpy(), g[n + '/map'], rtol=0, atol=MAP_TOL, err_msg=n)
        assert _psnr_ok(p, g[n + '/psnr']), (n, p, g[n + '/psnr'])


def _views_800(n=5, seed=11):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:800, 0:800].astype(np.float32) / 800
    gt, out = [], []
    for i in range(n):
        base = np.stack([0.5 + 0.4 * np.sin((3 + i) * x + c) * np.cos((2 + c) * y) for c in range(3)], -1)
        gt.append(base.astype(np.float32))
        out.append((base + rng.normal(0, 0.03 + 0.01 * i, base.shape)).astype(np.float32))
    return np.stack(out), np.stack(gt)


def test_hip_metrics_match_the_oracle_at_800x800_and_are_bitwise_reproducible():
    from directvoxgo_amd.metrics import image_metrics
    out, gt = _views_800()
    a, b = torch.from_numpy(out).cuda(), torch.from_numpy(gt).cuda()
    s, sse, m = image_metrics(a, b, return_map=True)
    s2, sse2, m2 = image_metrics(a, b, return_map=True)
    assert torch.equal(s, s2) and torch.equal(sse, sse2) and torch.equal(m, m2)       # run to run
    for i in range(len(out)):
        si, ssei, mi = image_metrics(a[i], b[i], return_map=True)                      # alone == member of the batch
        assert torch.equal(si[0], s[i]) and torch.equal(ssei[0], sse[i]) and torch.equal(mi[0], m[i]), i
        rs, rp, rm = MO.image_metrics(out[i], gt[i], return_map=True)
        assert abs(float(s[i]) - rs) <= SSIM_TOL, (i, float(s[i]), rs)
        p = -10 * np.log10(float(sse[i]) / (800 * 800 * 3))
        assert abs(p - rp) <= PSNR_TOL, (i, p, rp)
        assert float((m[i].cpu().double() - torch.from_numpy(rm)).abs().max()) <= MAP_TOL, i
    # a batch whose images sit at other places gives the same bits per image
    perm = [3, 0, 4]
    sp, ssep, _ = image_metrics(a[perm], b[perm])
    assert torch.equal(sp, s[perm]) and torch.equal(ssep, sse[perm])


def _scene():
    from directvoxgo_amd.dvgo import DirectVoxGO
    from directvoxgo_amd.scenes import pose_spherical, synthetic_scene
    sc = synthetic_scene(world=32, n_rays=64, seed=3, device='cuda')
    torch.manual_seed(8)
    m = DirectVoxGO(sc['xyz_min'], sc['xyz_max'], num_voxels=32 ** 3, num_voxels_base=32 ** 3, alpha_init=1e-2,
                    fast_color_thres=1e-4, rgbnet_dim=12, rgbnet_width=64, rgbnet_direct=True).cuda()
    with torch.no_grad():
        m.density.copy_(sc['density']); m.k0.copy_(sc['k0']); m.mask_cache.mask.copy_(sc['mask'])
    H = W = 40
    K = np.array([[55.0, 0, 20], [0, 55.0, 20], [0, 0, 1]], np.float32)
    poses = [pose_spherical(th, -30.0, 4.0).numpy() for th in (-120.0, -40.0, 10.0, 75.0, 160.0)]
    args = (m, poses, [(H, W)] * 5, [K] * 5, False, dict(near=sc['near'], far=sc['far'], bg=1, stepsize=0.5))
    return args


def _gt(rgbs):
    rng = np.random.default_rng(5)
    return np.clip(rgbs + rng.normal(0, 0.05, rgbs.shape), 0, 1).astype(np.float32)


def test_render_viewpoints_with_ground_truth(tmp_path, capsys):
    from directvoxgo_amd.render import evaluate_viewpoints, render_viewpoints
    args = _scene()
    rgbs, depths = render_viewpoints(*args, chunk=512)
    gt = _gt(rgbs)
    rgbs2, depths2 = render_viewpoints(*args, chunk=512, gt_imgs=gt, eval_ssim=True)
    assert np.array_equal(rgbs, rgbs2) and np.array_equal(depths, depths2)
    out = capsys.readouterr().out
    assert 'Testing psnr' in out and 'Testing ssim' in out
    res = evaluate_viewpoints(*args, chunk=512, gt_imgs=[torch.from_numpy(g).cuda() for g in gt], eval_ssim=True)
    assert np.array_equal(res['rgbs'], rgbs) and len(res['psnr']) == 5 and len(res['ssim']) == 5
    for i in range(5):
        rs, rp = MO.image_metrics(rgbs[i], gt[i])
        assert abs(res['ssim'][i] - rs) <= SSIM_TOL and abs(res['psnr'][i] - rp) <= PSNR_TOL, i
    assert 0 < min(res['ssim']) and max(res['ssim']) < 1
    res = evaluate_viewpoints(*args, chunk=512, gt_imgs=gt)                  # PSNR only
    assert res['ssim'] is None and len(res['psnr']) == 5
    res = evaluate_viewpoints(*args, chunk=512, gt_imgs=gt, render_factor=2, eval_ssim=True)   # run.py:116: no metrics
    assert res['psnr'] is None and res['ssim'] is None and res['rgbs'].shape == (5, 20, 20, 3)
    pytest.importorskip('PIL')
    from PIL import Image
    render_viewpoints(*args, chunk=512, savedir=str(tmp_path / 'png'))
    files = sorted(os.listdir(tmp_path / 'png'))
    assert files == ['%03d.png' % i for i in range(5)]
    from directvoxgo_amd.metrics import to8b
    assert np.array_equal(np.asarray(Image.open(tmp_path / 'png' / '002.png')), to8b(rgbs[2]))


@pytest.mark.timeout(300)
def test_evaluate_viewpoints_over_two_ranks_equals_one_process():
    import socket
    import torch.multiprocessing as mp
    from directvoxgo_amd.render import evaluate_viewpoints
    args = _scene()
    gt = _gt(evaluate_viewpoints(*args, chunk=512)['rgbs'])
    ref = evaluate_viewpoints(*args, chunk=512, gt_imgs=gt, eval_ssim=True)
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context('spawn')
    qin, qout = ctx.Queue(), ctx.Queue()
    procs = [ctx.Process(target=_eval_worker_io, args=(r, 2, port, qin, qout)) for r in range(2)]
    for p in procs:
        p.start()
    for _ in procs:
        qin.put(gt)
    got = [qout.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, psnrs, ssims in got:
        assert psnrs == ref['psnr'] and ssims == ref['ssim'], rank


def _eval_worker_io(rank, world, port, qin, qout):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from directvoxgo_amd.render import evaluate_viewpoints
    args = _scene()
    gt = qin.get(timeout=120)
    res = evaluate_viewpoints(*args, chunk=512, distributed=True, gt_imgs=gt, eval_ssim=True)
    qout.put((rank, res['psnr'], res['ssim']))
    dist.barrier()
    dist.destroy_process_group()
