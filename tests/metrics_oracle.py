"""numpy front-end of tests/metrics_oracle.c: SSIM and PSNR as the reference states them (lib/utils.py:88-134,
run.py:117), float32 products and float64 from the blur on.  TEST INFRASTRUCTURE ONLY (tests and tools/eval_bench.py);
the product never imports it.  Compiled with gcc on first use into the temporary directory."""
import ctypes
import hashlib
import os
import subprocess
import tempfile

import numpy as np

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'metrics_oracle.c')
_lib = None


def lib():
    global _lib
    if _lib is None:
        src = open(_SRC, 'rb').read()
        tag = hashlib.sha1(src).hexdigest()[:12]
        so = os.path.join(tempfile.gettempdir(), f'dvgo_metrics_oracle_{os.getuid()}_{tag}.so')
        if not os.path.exists(so):
            tmp = so + f'.{os.getpid()}'
            subprocess.check_call(['gcc', '-O2', '-std=c11', '-fPIC', '-shared', '-ffp-contract=off', '-fno-fast-math',
                                   '-Wall', '-o', tmp, _SRC, '-lm'])
            os.replace(tmp, so)
        _lib = ctypes.CDLL(so)
        _lib.ora_image_metrics.restype = ctypes.c_int
    return _lib


def taps(filter_size, filter_sigma):
    """lib/utils.py:101-105"""
    hw = filter_size // 2
    shift = (2 * hw - filter_size + 1) / 2
    f_i = ((np.arange(filter_size) - hw + shift) / filter_sigma) ** 2
    filt = np.exp(-0.5 * f_i)
    return filt / np.sum(filt)


def image_metrics(img0, img1, max_val=1.0, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, return_map=False):
    """-> (ssim, psnr[, map float64 [H-fs+1, W-fs+1, 3]]) of one [H, W, 3] pair."""
    a = np.ascontiguousarray(img0, dtype=np.float32)
    b = np.ascontiguousarray(img1, dtype=np.float32)
    assert a.ndim == 3 and a.shape[-1] == 3 and a.shape == b.shape
    H, W = a.shape[:2]
    f = np.ascontiguousarray(taps(filter_size, filter_sigma), dtype=np.float64)
    m = np.empty((H - filter_size + 1, W - filter_size + 1, 3), np.float64) if return_map else None
    s, e = ctypes.c_double(), ctypes.c_double()
    dp = ctypes.POINTER(ctypes.c_double)
    fp = ctypes.POINTER(ctypes.c_float)
    rc = lib().ora_image_metrics(a.ctypes.data_as(fp), b.ctypes.data_as(fp), ctypes.c_int(H), ctypes.c_int(W),
                                 f.ctypes.data_as(dp), ctypes.c_int(filter_size), ctypes.c_double((k1 * max_val) ** 2),
                                 ctypes.c_double((k2 * max_val) ** 2), m.ctypes.data_as(dp) if m is not None else None,
                                 ctypes.byref(s), ctypes.byref(e))
    if rc != 0:
        raise ValueError(f'ora_image_metrics: {rc}')
    n_map = (H - filter_size + 1) * (W - filter_size + 1) * 3
    mse = e.value / (H * W * 3)
    psnr = float('inf') if mse == 0 else -10.0 * np.log10(mse)
    out = (s.value / n_map, psnr)
    return out + (m,) if return_map else out
