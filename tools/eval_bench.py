"""Scoring rendered views (SSIM + PSNR on the device, csrc/metrics.hip) next to rendering them: the scene of
tools/render_bench.py (256^3 grid, 800x800 views).  Ground truth is a render of the same model with its k0 grid perturbed,
so SSIM is well below 1.  Prints one JSON line:

  render_ms_per_view           render_viewpoints, host clock around synchronised work
  metric_ms_per_view_batch     image_metrics on all views in one call (device events, warmed up, averaged)
  metric_ms_per_view_single    image_metrics one view at a time (device events)
  gt_upload_ms_per_view        numpy float32 view -> device (pageable copy, as evaluate_viewpoints does)
  host_scipy_ms_one_view       the reference's scipy statement of SSIM (lib/utils.py:88-134) on one view, with the CPU
                               model and thread count
  max_abs_dssim / max_abs_dpsnr  device results against the CPU metrics oracle (tests/metrics_oracle.c)

Kernel times come from a separate run under the kernel tracer:
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/eval_bench.py --trace
  python tools/eval_bench.py --stats OUT/.../kernel_stats.csv [--views 5]
The second form prints the metric kernels' average times and the share of the HBM floor (bytes the batch must read over
kernel time; 8 TB/s peak, MI355X_MICROARCH).
"""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

HBM_PEAK = 8.0e12


def bytes_read(n, H, W):
    return 2 * n * H * W * 3 * 4


def stats(path, n, H, W):
    """kernel_stats.csv of a --trace run (batch calls of n views only) -> kernel times and the HBM-floor share."""
    import csv
    rows = list(csv.DictReader(open(path)))
    tile = [r for r in rows if 'metrics_tile_kernel' in r['Name']]
    red = [r for r in rows if 'metrics_reduce_kernel' in r['Name']]
    assert tile and red, 'metric kernels not in the trace'
    t_tile, t_red = float(tile[0]['AverageNs']) * 1e-9, float(red[0]['AverageNs']) * 1e-9
    floor = bytes_read(n, H, W) / HBM_PEAK
    return {'views': n, 'hw': H, 'calls': int(tile[0]['Calls']), 'tile_kernel_us': round(t_tile * 1e6, 2),
            'reduce_kernel_us': round(t_red * 1e6, 2), 'kernel_us_per_view': round((t_tile + t_red) * 1e6 / n, 2),
            'bytes_read': bytes_read(n, H, W), 'hbm_floor_us': round(floor * 1e6, 2),
            'share_of_hbm_floor': round(floor / (t_tile + t_red), 4)}


def scipy_ssim(img0, img1, max_val, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03):
    """The reference's host statement (lib/utils.py:88-134), restated for timing."""
    import scipy.signal
    hw = filter_size // 2
    shift = (2 * hw - filter_size + 1) / 2
    f_i = ((np.arange(filter_size) - hw + shift) / filter_sigma) ** 2
    filt = np.exp(-0.5 * f_i)
    filt /= np.sum(filt)

    def filt_fn(z):
        return np.stack([scipy.signal.convolve2d(scipy.signal.convolve2d(z[..., i], filt[:, None], mode='valid'),
                                                 filt[None, :], mode='valid') for i in range(z.shape[-1])], -1)
    mu0, mu1 = filt_fn(img0), filt_fn(img1)
    mu00, mu11, mu01 = mu0 * mu0, mu1 * mu1, mu0 * mu1
    s00 = np.maximum(0., filt_fn(img0 ** 2) - mu00)
    s11 = np.maximum(0., filt_fn(img1 ** 2) - mu11)
    s01 = filt_fn(img0 * img1) - mu01
    s01 = np.sign(s01) * np.minimum(np.sqrt(s00 * s11), np.abs(s01))
    c1, c2 = (k1 * max_val) ** 2, (k2 * max_val) ** 2
    return np.mean((2 * mu01 + c1) * (2 * s01 + c2) / ((mu00 + mu11 + c1) * (s00 + s11 + c2)))


def cpu_model():
    try:
        for ln in open('/proc/cpuinfo'):
            if ln.startswith('model name'):
                return ln.split(':', 1)[1].strip()
    except OSError:
        pass
    return platform.processor()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--world', type=int, default=256)
    ap.add_argument('--views', type=int, default=5)
    ap.add_argument('--hw', type=int, default=800)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--trace', action='store_true', help='only the metric calls (for a kernel-trace run)')
    ap.add_argument('--stats', help='kernel_stats.csv of a --trace run: kernel times and HBM-floor share')
    args = ap.parse_args()
    H = W = args.hw
    if args.stats:
        print(json.dumps(stats(args.stats, args.views, H, W)))
        return

    import torch
    from directvoxgo_amd.dvgo import DirectVoxGO
    from directvoxgo_amd.metrics import image_metrics
    from directvoxgo_amd.render import render_viewpoints
    from directvoxgo_amd.scenes import pose_spherical, synthetic_scene
    assert torch.cuda.is_available(), 'eval_bench needs a GPU'

    sc = synthetic_scene(world=args.world, n_rays=8, device='cuda')
    torch.manual_seed(0)
    m = DirectVoxGO(sc['xyz_min'], sc['xyz_max'], num_voxels=args.world ** 3, num_voxels_base=args.world ** 3,
                    alpha_init=1e-2, fast_color_thres=1e-4, rgbnet_dim=12, rgbnet_width=128, rgbnet_direct=True).cuda()
    with torch.no_grad():
        m.density.copy_(sc['density']); m.k0.copy_(sc['k0']); m.mask_cache.mask.copy_(sc['mask'])
        # the freshly initialised colour head barely depends on k0 (a k0 perturbation alone left SSIM at 0.99996):
        # a steeper output layer makes the perturbed render a ground truth that differs visibly
        m.rgbnet[-1].weight.mul_(30.0)
    K = np.array([[1111.11 * W / 800, 0, 0.5 * W], [0, 1111.11 * H / 800, 0.5 * H], [0, 0, 1]], np.float32)
    poses = [pose_spherical(40.0 * i - 60, -30.0, 4.0).numpy() for i in range(args.views)]
    rk = dict(near=2.0, far=6.0, bg=1, stepsize=0.5, inverse_y=False)
    n = len(poses)
    HWs, Ks = [(H, W)] * n, [K] * n

    render_viewpoints(m, poses[:1], [(H, W)], [K], False, rk)                     # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rgbs, _ = render_viewpoints(m, poses, HWs, Ks, False, rk)
    torch.cuda.synchronize()
    render_ms = (time.perf_counter() - t0) / n * 1e3
    k0 = m.k0.detach().clone()
    with torch.no_grad():
        g = torch.Generator(device='cuda').manual_seed(1)
        m.k0.add_(1.0 * torch.randn(m.k0.shape, device='cuda', generator=g))
    gt, _ = render_viewpoints(m, poses, HWs, Ks, False, rk)
    with torch.no_grad():
        m.k0.copy_(k0)
    a = torch.from_numpy(rgbs).cuda()
    b = torch.from_numpy(gt).cuda()

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    if args.trace:
        for _ in range(args.reps):
            image_metrics(a, b)
        torch.cuda.synchronize()
        return

    batch_ms = timed(lambda: image_metrics(a, b), args.reps) / n
    single_ms = timed(lambda: [image_metrics(a[i], b[i]) for i in range(n)], args.reps) / n
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.reps):
        for i in range(n):
            torch.from_numpy(gt[i]).cuda()
    torch.cuda.synchronize()
    upload_ms = (time.perf_counter() - t0) / (args.reps * n) * 1e3

    t0 = time.perf_counter()
    ref_scipy = scipy_ssim(rgbs[0], gt[0], 1.0)
    scipy_ms = (time.perf_counter() - t0) * 1e3

    import metrics_oracle as MO
    s, sse, _ = image_metrics(a, b)
    s, sse = s.cpu().numpy(), sse.cpu().numpy()
    dssim, dpsnr = 0.0, 0.0
    for i in range(n):
        rs, rp = MO.image_metrics(rgbs[i], gt[i])
        p = -10 * np.log10(sse[i] / (H * W * 3))
        dssim, dpsnr = max(dssim, abs(s[i] - rs)), max(dpsnr, abs(p - rp))
    print(json.dumps({
        'views': n, 'hw': H, 'world': args.world,
        'render_ms_per_view': round(render_ms, 3),
        'metric_ms_per_view_batch': round(batch_ms, 4),
        'metric_ms_per_view_single': round(single_ms, 4),
        'metric_share_of_render_batch': round(batch_ms / render_ms, 5),
        'gt_upload_ms_per_view': round(upload_ms, 4),
        'host_scipy_ms_one_view': round(scipy_ms, 1),
        'host_cpu': cpu_model(), 'host_threads': os.cpu_count(),
        'ssim': [round(float(x), 6) for x in s], 'psnr': [round(float(-10 * np.log10(e / (H * W * 3))), 4) for e in sse],
        'scipy_minus_device_ssim_view0': float(ref_scipy - s[0]),
        'max_abs_dssim_vs_oracle': float(dssim), 'max_abs_dpsnr_vs_oracle': float(dpsnr),
    }))


if __name__ == '__main__':
    main()
