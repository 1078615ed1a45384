"""Image metrics of rendered views on the device: SSIM and PSNR as the reference reports them.

  ssim      lib/utils.py:88-134  rgb_ssim (same signature); one HIP launch pair for a whole batch
                                 (csrc/metrics.hip: dvgo_image_metrics)
  psnr      run.py:117           -10 log10(mean((img - gt)^2)); identical images give +inf, as numpy does
  to8b      lib/utils.py:18
  mse2psnr  lib/utils.py:17

Inputs are [H, W, 3] or [n, H, W, 3] fp32 device tensors, or numpy arrays (uploaded to the current device).  A single
image gives Python floats, a batch an [n] float64 numpy array.  Deliberate difference: images smaller than the filter
(the reference's empty mean, nan) raise ValueError.  The kernel holds filters of up to 16 taps.
"""
import ctypes

import numpy as np
import torch

from . import _lib as L
from ._lib import _i64, _int, ptr

FILTER_SIZE_MAX = 16          # MT_FS_MAX of csrc/metrics.hip

mse2psnr = lambda x: -10. * torch.log10(x)
to8b = lambda x: (255 * np.clip(x, 0, 1)).astype(np.uint8)


def gaussian_taps(filter_size, filter_sigma):
    """The 1-D blur filter in float64, exactly as lib/utils.py:101-105 builds it."""
    hw = filter_size // 2
    shift = (2 * hw - filter_size + 1) / 2
    f_i = ((np.arange(filter_size) - hw + shift) / filter_sigma) ** 2
    filt = np.exp(-0.5 * f_i)
    filt /= np.sum(filt)
    return filt


def _as_batch(x, name, device=None):
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        x = x.to(device if device is not None else torch.device('cuda', torch.cuda.current_device()))
    L.check_f32(x, name)
    if x.dim() == 3:
        x = x[None]
    x = x.contiguous()
    L.check_input(x, name)
    return x


def image_metrics(img0, img1, max_val=1.0, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, return_map=False):
    """-> (ssim [n] float64 tensor, sse [n] float64 tensor, map [n, H-fs+1, W-fs+1, 3] fp32 or None), on the device.

    sse is the sum of squared differences over all H*W*3 values.  Enqueued on torch's current stream; nothing is copied to
    the host."""
    shape0, shape1 = tuple(np.shape(img0))[-3:], tuple(np.shape(img1))[-3:]
    if shape0 != shape1 or np.ndim(img0) != np.ndim(img1):
        raise ValueError(f'img0 {tuple(np.shape(img0))} and img1 {tuple(np.shape(img1))} differ in shape')
    if len(shape0) != 3 or shape0[-1] != 3:
        raise ValueError(f'images must be [H, W, 3] or [n, H, W, 3], got {tuple(np.shape(img0))}')
    H, W = int(shape0[0]), int(shape0[1])
    fs = int(filter_size)
    if fs < 1:
        raise ValueError(f'filter_size must be >= 1, got {fs}')
    if H < fs or W < fs:
        raise ValueError(f'image {H}x{W} is smaller than the {fs}-tap filter: the SSIM map would be empty '
                         '(the reference returns nan here)')
    if fs > FILTER_SIZE_MAX:
        raise ValueError(f'filter_size {fs} > {FILTER_SIZE_MAX} is not supported by the kernel')
    a = _as_batch(img0, 'img0')
    b = _as_batch(img1, 'img1', device=a.device)
    if a.device != b.device:
        raise ValueError('img0 and img1 live on different devices')
    n = a.shape[0]
    f = gaussian_taps(fs, filter_sigma)
    taps = (ctypes.c_double * fs)(*f.tolist())
    c1, c2 = (k1 * max_val) ** 2, (k2 * max_val) ** 2
    ssim_sum = torch.empty(n, dtype=torch.float64, device=a.device)
    sse = torch.empty(n, dtype=torch.float64, device=a.device)
    smap = torch.empty((n, H - fs + 1, W - fs + 1, 3), dtype=torch.float32, device=a.device) if return_map else None
    lib = L.lib()
    nbytes = lib.dvgo_image_metrics_workspace_bytes(_i64(n), _int(H), _int(W), _int(fs))
    if nbytes < 0:
        raise RuntimeError(f'dvgo_image_metrics_workspace_bytes failed: {L._ERR.get(nbytes, nbytes)}')
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=a.device)
    with L.device_of(a):
        L.call('dvgo_image_metrics', ptr(a), ptr(b), _i64(n), _int(H), _int(W), taps, _int(fs), ctypes.c_double(c1),
               ctypes.c_double(c2), ptr(ssim_sum), ptr(sse), ptr(smap), ptr(ws), _i64(ws.numel()), L.stream_of(a))
    return ssim_sum / float((H - fs + 1) * (W - fs + 1) * 3), sse, smap


def _psnr_of(sse, n_values):
    mse = sse / n_values
    with np.errstate(divide='ignore'):
        return -10. * np.log10(mse)


def _is_single(x):
    return (x.dim() if isinstance(x, torch.Tensor) else np.ndim(x)) == 3


def _result(x, single):
    return float(x[0]) if single else x


def ssim(img0, img1, max_val, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, return_map=False):
    """lib/utils.py:88-134 rgb_ssim on the device.  -> float ([H,W,3]) or [n] float64 array ([n,H,W,3]); with
    return_map, the SSIM map (fp32 device tensor, [H-fs+1, W-fs+1, 3] or batched) as in the reference."""
    single = _is_single(img0)
    s, _, m = image_metrics(img0, img1, max_val, filter_size, filter_sigma, k1, k2, return_map=return_map)
    if return_map:
        return m[0] if single else m
    return _result(s.cpu().numpy(), single)


def psnr(img, gt):
    """run.py:117  -10 log10(mean((img - gt)^2)) on the device (the squared error of csrc/metrics.hip; the SSIM it also
    computes with a 1-tap filter is discarded).  -> float, or [n] float64 array for a batch."""
    single = _is_single(img)
    _, sse, _ = image_metrics(img, gt, filter_size=1, filter_sigma=1.0)
    H, W = np.shape(img)[-3:-1]
    return _result(_psnr_of(sse.cpu().numpy(), H * W * 3), single)
