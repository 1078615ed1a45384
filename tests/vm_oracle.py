"""Oracle of the vector-matrix sampler (csrc/vm.hip; include/dvgo_hip.h, the VM block), numpy.

Coordinates, floors and weights in float32, operation for operation what the kernels do (tests/triplane_oracle.py's `_axis`
and `corners`); values and sums in float64.  Per sample m, plane / line s and component r:
    p = sum over the plane's corners inside of k * v          k = wh * ww (float32)
    l = sum over the line's nodes inside of w * v_line        w = (f + 1) - g, g - f (float32)
    out[m, s R + r] = p * l
Line xy runs along world x, yz along z, zx along y: the axis its plane does not see.

forward  -> value [M, 3R] and A = (sum |k v|) (sum |w v_line|) per output.
backward -> per plane texel: grad = sum k l g, A = sum |k| (sum |w v_line|) |g|, and the count n of contributions;
            per line node:   grad = sum w p g, A = sum |w| (sum |k v|) |g|, and n.
line32   -> the line sample in float32 with correctly rounded fused multiply-adds: the kernel's bits.
"""
import numpy as np

import triplane_oracle as TO
from interp_oracle import fma32

KEYS = TO.KEYS
LINE_AXIS = {'xy': 0, 'yz': 2, 'zx': 1}
U = TO.U
f32 = np.float32


def _chw(p):
    p = np.asarray(p)
    return p[0] if p.ndim == 4 else p


def _rn(ln):
    """[1, R, N, 1] or [R, N] -> [R, N]"""
    ln = np.asarray(ln)
    return ln[0, :, :, 0] if ln.ndim == 4 else ln


def nodes(key, N, xyz, mn, mx):
    """The two nodes of line `key` at every sample: -> idx [2, M] int64, w [2, M] float32, ok [2, M] bool."""
    a = LINE_AXIS[key]
    n0, w0, w1 = TO._axis(xyz[:, a], mn[a], mx[a], N)
    idx = np.stack([n0, n0 + 1])
    w = np.stack([w0, w1])
    assert w.dtype == f32
    return idx, w, (idx >= 0) & (idx < N)


def _plane_parts(key, p, xyz, mn, mx):
    """p [R, H, W] float64 -> value [M, R], magnitude [M, R]"""
    R, H, W = p.shape
    ih, iw, k, ok = TO.corners(key, H, W, xyz, mn, mx)
    v = np.zeros((xyz.shape[0], R)); a = np.zeros((xyz.shape[0], R))
    for n in range(4):
        term = p[:, np.clip(ih[n], 0, H - 1), np.clip(iw[n], 0, W - 1)].T * (k[n].astype(np.float64) * ok[n])[:, None]
        v += term; a += np.abs(term)
    return v, a


def _line_parts(key, ln, xyz, mn, mx):
    """ln [R, N] float64 -> value [M, R], magnitude [M, R]"""
    R, N = ln.shape
    idx, w, ok = nodes(key, N, xyz, mn, mx)
    v = np.zeros((xyz.shape[0], R)); a = np.zeros((xyz.shape[0], R))
    for n in range(2):
        term = ln[:, np.clip(idx[n], 0, N - 1)].T * (w[n].astype(np.float64) * ok[n])[:, None]
        v += term; a += np.abs(term)
    return v, a


def forward(planes, lines, xyz, mn, mx):
    """planes {'xy','yz','zx'} of [1,R,H,W], lines likewise of [1,R,N,1], float32 -> (value, A) [M, 3R], float64."""
    xyz = np.asarray(xyz, f32)
    vals, mags = [], []
    for key in KEYS:
        pv, pa = _plane_parts(key, _chw(planes[key]).astype(np.float64), xyz, mn, mx)
        lv, la = _line_parts(key, _rn(lines[key]).astype(np.float64), xyz, mn, mx)
        vals.append(pv * lv); mags.append(pa * la)
    return np.concatenate(vals, 1), np.concatenate(mags, 1)


def backward(planes, lines, xyz, mn, mx, grad_out):
    """-> ({key: (grad [R,H,W], A [R,H,W], n [H,W])}, {key: (grad [R,N], A [R,N], n [N])}), float64 / int64."""
    xyz = np.asarray(xyz, f32)
    g_all = np.asarray(grad_out, np.float64)
    gp, gl = {}, {}
    for s, key in enumerate(KEYS):
        p, ln = _chw(planes[key]).astype(np.float64), _rn(lines[key]).astype(np.float64)
        R, H, W = p.shape
        N = ln.shape[1]
        g = g_all[:, s * R:(s + 1) * R]
        pv, pa = _plane_parts(key, p, xyz, mn, mx)
        lv, la = _line_parts(key, ln, xyz, mn, mx)
        ih, iw, k, ok = TO.corners(key, H, W, xyz, mn, mx)
        grad = np.zeros((H * W, R)); A = np.zeros((H * W, R)); cnt = np.zeros(H * W, np.int64)
        for n in range(4):
            sel = ok[n]
            flat = ih[n][sel] * W + iw[n][sel]
            kk = k[n][sel].astype(np.float64)[:, None]
            np.add.at(grad, flat, kk * lv[sel] * g[sel])
            np.add.at(A, flat, np.abs(kk) * la[sel] * np.abs(g[sel]))
            np.add.at(cnt, flat, 1)
        gp[key] = (grad.reshape(H, W, R).transpose(2, 0, 1), A.reshape(H, W, R).transpose(2, 0, 1), cnt.reshape(H, W))
        idx, w, okn = nodes(key, N, xyz, mn, mx)
        grad = np.zeros((N, R)); A = np.zeros((N, R)); cnt = np.zeros(N, np.int64)
        for n in range(2):
            sel = okn[n]
            ww = w[n][sel].astype(np.float64)[:, None]
            np.add.at(grad, idx[n][sel], ww * pv[sel] * g[sel])
            np.add.at(A, idx[n][sel], np.abs(ww) * pa[sel] * np.abs(g[sel]))
            np.add.at(cnt, idx[n][sel], 1)
        gl[key] = (grad.T, A.T, cnt)
    return gp, gl


def line32(key, ln, xyz, mn, mx):
    """The line sample as the kernel computes it, float32: l = 0; l = fma(v[f], w0, l); l = fma(v[f+1], w1, l), nodes
    outside skipped.  ln [1,R,N,1] or [R,N] float32 -> [M, R] float32."""
    ln = _rn(ln).astype(f32)
    R, N = ln.shape
    idx, w, ok = nodes(key, N, np.asarray(xyz, f32), mn, mx)
    acc = np.zeros((xyz.shape[0], R), f32)
    for n in range(2):
        v = ln[:, np.clip(idx[n], 0, N - 1)].T
        acc = np.where(ok[n][:, None], fma32(v, np.broadcast_to(w[n][:, None], v.shape), acc), acc)
    return acc


def torch_restatement(planes, lines, xyz, mn, mx):
    """The same function in torch ops, in the dtype of its inputs (float64 on the CPU in the tests): six F.grid_sample
    (bilinear, align_corners=True, zero padding), product, cat.  planes / lines: dicts of tensors [1,R,H,W] / [1,R,N,1];
    differentiable."""
    import torch
    import torch.nn.functional as F
    pairs = {'xy': [0, 1], 'yz': [1, 2], 'zx': [2, 0]}           # of the flipped triple (n_z, n_y, n_x): (columns, rows)
    x = xyz.reshape(1, 1, -1, 3)
    ind = ((x - mn) / (mx - mn)).flip((-1,)) * 2 - 1
    out = []
    for key in KEYS:
        p = F.grid_sample(planes[key], ind[..., pairs[key]], mode='bilinear', align_corners=True)[0, :, 0, :].T
        along = ind[..., [2 - LINE_AXIS[key]]]                   # the line's axis addresses its rows; its one column is 0
        grid = torch.cat([torch.zeros_like(along), along], -1)
        ln = F.grid_sample(lines[key], grid, mode='bilinear', align_corners=True)[0, :, 0, :].T
        out.append(p * ln)
    return torch.cat(out, -1)
