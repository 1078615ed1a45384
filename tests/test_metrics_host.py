"""CPU: the image-metrics feature without a GPU -- the C-ABI entry's argument checks, the wait-state / packed-fp32 lint and
scratch use of csrc/metrics.hip, the metrics oracle against the reference's own SSIM / PSNR (tests/golden/metrics.npz),
and the host logic of render_viewpoints' metric arguments."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, load_golden

HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


@pytest.fixture(scope='module')
def so_path():
    from directvoxgo_amd import build
    return build.build(verbose=False)


def test_image_metrics_argument_validation_returns_error_codes_before_any_launch(so_path):
    lib = ctypes.CDLL(so_path)
    lib.dvgo_image_metrics_workspace_bytes.restype = ctypes.c_int64
    vp, i64, i32, d = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double
    null, one = vp(0), vp(16)          # `one`: any non-null value, rejected before it could be dereferenced
    taps = (ctypes.c_double * 16)(*([1.0 / 16] * 16))

    def call(img, n, H, W, fs, out=one, ws=one, ws_bytes=1 << 30, t=taps):
        return lib.dvgo_image_metrics(img, img, i64(n), i32(H), i32(W), t, i32(fs), d(1e-4), d(9e-4), out, out, null,
                                      ws, i64(ws_bytes), null)

    assert call(null, 0, 32, 32, 11) == 0                     # n == 0: no-op
    assert call(null, -1, 32, 32, 11) == -1                   # negative size
    assert call(one, 2, -4, 32, 11) == -1
    assert call(one, 2, 32, 0, 11) == -1
    assert call(one, 2, 10, 32, 11) == -1                     # H < filter_size (the reference: nan)
    assert call(one, 2, 32, 10, 11) == -1                     # W < filter_size
    assert call(one, 2, 32, 32, 0) == -1
    assert call(one, 2, 32, 32, 17) == -2                     # beyond the kernel's 16 taps
    assert call(one, 1, 30000, 30000, 11) == -2               # H*W*3 >= 2^31
    assert call(null, 2, 32, 32, 11) == -1                    # null images
    assert call(one, 2, 32, 32, 11, out=null) == -1           # null outputs
    assert call(one, 2, 32, 32, 11, ws=null) == -1            # null workspace
    assert call(one, 2, 32, 32, 11, t=None) == -1             # null taps
    need = lib.dvgo_image_metrics_workspace_bytes(i64(2), i32(32), i32(32), i32(11))
    assert need > 0
    assert call(one, 2, 32, 32, 11, ws_bytes=need - 1) == -1  # short workspace
    assert lib.dvgo_image_metrics_workspace_bytes(i64(2), i32(8), i32(32), i32(11)) == -1
    assert lib.dvgo_image_metrics_workspace_bytes(i64(2), i32(64), i32(64), i32(40)) == -2


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='needs hipcc')
def test_metrics_unit_obeys_the_wait_state_rules_and_uses_no_scratch(tmp_path):
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    import hazard_lint as H
    from directvoxgo_amd.build import FLAGS
    src = os.path.join(REPO, 'directvoxgo_amd', 'csrc', 'metrics.hip')
    flags = [f for f in FLAGS if f not in ('-shared', '-Wall', '-Wno-unused-function')]
    asm = str(tmp_path / 'metrics.s')
    p = subprocess.run([HIPCC] + flags + ['-S', '--cuda-device-only', '-Rpass-analysis=kernel-resource-usage', src, '-o', asm],
                       check=True, capture_output=True, text=True)
    bad, n_kernels = [], 0
    for name, items in H.parse(asm).items():
        if not any(k == 'ins' for k, _ in items):
            continue
        n_kernels += 1
        bad += H.check_kernel(name, items)[0]
    assert n_kernels == 2
    assert not bad, '\n'.join(bad[:20])
    scratch = re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', p.stderr)
    assert len(scratch) == 2 and all(s == '0' for s in scratch), p.stderr


def _golden_cases():
    g = load_golden('metrics')
    return g, [str(n) for n in g['names']]


def test_metrics_oracle_matches_the_reference_fixture():
    import metrics_oracle as MO
    g, names = _golden_cases()
    assert len(names) >= 14
    for n in names:
        max_val, fs, sigma = g[n + '/params']
        s, p, m = MO.image_metrics(g[n + '/img0'], g[n + '/img1'], max_val, int(fs), sigma, return_map=True)
        assert m.shape == g[n + '/map'].shape, n
        assert abs(s - g[n + '/ssim']) <= 1e-9, (n, s, g[n + '/ssim'])
        np.testing.assert_allclose(m, g[n + '/map'], rtol=0, atol=1e-8, err_msg=n)
        if np.isinf(g[n + '/psnr']):
            assert p == g[n + '/psnr'], n
        else:
            assert abs(p - g[n + '/psnr']) <= 1e-4, (n, p, g[n + '/psnr'])
    assert g['identical/ssim'] == 1.0 and np.isinf(g['identical/psnr'])
    assert (g['negative_cov/map'] < 0).any()       # the sign clip is exercised


def test_gaussian_taps_are_the_reference_filter():
    import metrics_oracle as MO
    from directvoxgo_amd.metrics import gaussian_taps
    for fs, sigma in ((11, 1.5), (7, 1.5), (8, 1.5), (11, 0.8), (1, 1.0)):
        f = gaussian_taps(fs, sigma)
        assert np.array_equal(f, MO.taps(fs, sigma))
        assert np.array_equal(f, f[::-1])          # symmetric: convolve2d's flip changes nothing


def test_render_factor_matches_the_reference_expression():
    from directvoxgo_amd.render import apply_render_factor
    HW = np.array([[800, 800], [801, 603]])
    Ks = np.array([[[1111.1, 0, 400.5], [0, 1111.1, 399.7], [0, 0, 1]]] * 2, np.float32)
    for f in (2, 3, 4):
        hw, ks = apply_render_factor(HW, Ks, f)
        eh, ek = np.copy(HW), np.copy(Ks)               # run.py:65-69
        eh //= f
        ek[:, :2, :3] //= f
        assert np.array_equal(hw, eh) and np.array_equal(ks, ek)
        assert HW[0, 0] == 800 and Ks[0, 0, 0] == np.float32(1111.1)      # copies: the inputs are untouched
    hw, ks = apply_render_factor(HW, Ks, 0)
    assert hw is HW and ks is Ks


@pytest.mark.parametrize('which', ['eval_lpips_alex', 'eval_lpips_vgg'])
def test_lpips_is_not_provided(which):
    from directvoxgo_amd.render import evaluate_viewpoints, render_viewpoints
    for fn in (render_viewpoints, evaluate_viewpoints):
        with pytest.raises(NotImplementedError, match='LPIPS'):
            fn(None, [np.eye(4)], [(8, 8)], [np.eye(3)], False, {}, gt_imgs=[np.zeros((8, 8, 3))], **{which: True})


def test_ssim_of_images_smaller_than_the_filter_raises():
    from directvoxgo_amd import metrics
    a = np.zeros((10, 40, 3), np.float32)
    with pytest.raises(ValueError, match='smaller than'):
        metrics.ssim(a, a, max_val=1)
    with pytest.raises(ValueError, match='smaller than'):
        metrics.ssim(a[None], a[None], max_val=1, filter_size=41)
    with pytest.raises(ValueError, match='differ in shape'):
        metrics.ssim(a, a[:, :30], max_val=1)


def test_to8b_and_mse2psnr_are_the_reference_expressions():
    import torch
    from directvoxgo_amd.metrics import mse2psnr, to8b
    x = np.array([-0.5, 0.0, 0.5, 0.999, 1.0, 2.0], np.float32)
    assert np.array_equal(to8b(x), (255 * np.clip(x, 0, 1)).astype(np.uint8))
    assert float(mse2psnr(torch.tensor(0.01))) == pytest.approx(20.0)
