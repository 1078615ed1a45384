"""Generate tests/golden/metrics.npz by RUNNING THE REFERENCE's own SSIM (lib/utils.py:88-134 rgb_ssim, scipy on the
host) and its PSNR expression (run.py:117, on float32 arrays).

The reference is imported through make_golden.import_reference() (a scratch copy, JIT loader and imageio/cv2 stubbed), never
in place.  Runs only where the reference tree exists; the fixture it writes is committed.

Usage:  python tests/golden/make_golden_metrics.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402


def smooth(rng, H, W):
    """a smooth field (low-frequency cosines) in [0, 1]"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros((H, W, 3))
    for c in range(3):
        for _ in range(3):
            fy, fx, ph = rng.uniform(0.02, 0.15), rng.uniform(0.02, 0.15), rng.uniform(0, 2 * np.pi)
            out[..., c] += np.cos(fy * y + fx * x + ph)
    return (0.5 + out / 6.0).astype(np.float32)


def cases(rng):
    """(name, img0, img1, max_val, filter_size, filter_sigma)"""
    out = []
    for H, W in ((11, 11), (37, 53), (64, 48)):
        out.append((f'random_{H}x{W}', rng.random((H, W, 3), dtype=np.float32), rng.random((H, W, 3), dtype=np.float32),
                    1.0, 11, 1.5))
        s = smooth(rng, H, W)
        out.append((f'smooth_noise_{H}x{W}', s, (s + 0.05 * rng.standard_normal((H, W, 3))).astype(np.float32), 1.0, 11, 1.5))
    s = smooth(rng, 24, 28)
    out.append(('identical', s, s.copy(), 1.0, 11, 1.5))
    out.append(('constant', np.full((24, 30, 3), 0.25, np.float32), np.full((24, 30, 3), 0.75, np.float32), 1.0, 11, 1.5))
    out.append(('negative_cov', s, (1.0 - s).astype(np.float32), 1.0, 11, 1.5))
    out.append(('outside_01', (s * 1.1 - 0.05).astype(np.float32),
                (s + 0.08 * rng.standard_normal(s.shape) + 0.02).astype(np.float32), 1.0, 11, 1.5))
    t = smooth(rng, 26, 30)
    n = (t + 0.04 * rng.standard_normal(t.shape)).astype(np.float32)
    out.append(('fs7', t, n, 1.0, 7, 1.5))
    out.append(('fs8', t, n, 1.0, 8, 1.5))
    out.append(('sigma08', t, n, 1.0, 11, 0.8))
    out.append(('maxval2', (2 * t).astype(np.float32), (2 * n).astype(np.float32), 2.0, 11, 1.5))
    return out


def main():
    R = make_golden.import_reference()
    import lib.utils as U
    rng = np.random.default_rng(20261015)
    arrs = {}
    names = []
    for name, a, b, max_val, fs, sigma in cases(rng):
        ssim_map = U.rgb_ssim(a, b, max_val, filter_size=fs, filter_sigma=sigma, return_map=True)
        ssim = U.rgb_ssim(a, b, max_val, filter_size=fs, filter_sigma=sigma)
        with np.errstate(divide='ignore'):
            psnr = -10. * np.log10(np.mean(np.square(a - b)))         # run.py:117
        names.append(name)
        arrs[name + '/img0'] = a
        arrs[name + '/img1'] = b
        arrs[name + '/params'] = np.array([max_val, fs, sigma], np.float64)
        arrs[name + '/ssim'] = np.float64(ssim)
        arrs[name + '/map'] = ssim_map.astype(np.float64)
        arrs[name + '/psnr'] = np.float64(psnr)
    arrs['names'] = np.array(names)
    path = os.path.join(HERE, 'metrics.npz')
    np.savez_compressed(path, **arrs)
    print('wrote', path, os.path.getsize(path) // 1024, 'KiB', '(reference copy in', R.scratch + ')')


if __name__ == '__main__':
    main()
