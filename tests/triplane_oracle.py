"""Oracle of the tri-plane sampler (csrc/triplane.hip; lib/tri_dvgo.py:456-469), numpy.

Coordinates, floor and weights in float32, operation for operation what the kernels do: per axis
g = ((((p - mn) / (mx - mn)) * 2 - 1) + 1) / 2 * (size - 1), f = floor(g), w0 = (f + 1) - g, w1 = g - f, a corner's weight
wh * ww.  Values and sums in float64.  Corners outside a plane are skipped (zero padding, align_corners=True).
Plane xy has its rows along world y and its columns along z, yz rows x / columns y, zx rows z / columns x.

forward  -> value [M, 3C] (concat) or [M, C] (sum), and A = sum |w * v| of the terms of each output.
backward -> per plane: the texel gradient [C, H, W], A = sum |w * g| and the count n of contributions, per texel.
"""
import numpy as np

KEYS = ('xy', 'yz', 'zx')
AXES = {'xy': (1, 2), 'yz': (0, 1), 'zx': (2, 0)}
U = 2.0 ** -24
f32 = np.float32


def _axis(p, mn, mx, size):
    """float32: floor index (int64) and the two weights of one axis."""
    p, mn, mx = p.astype(f32), f32(mn), f32(mx)
    u = (p - mn) / (mx - mn)
    c = u * f32(2.0) - f32(1.0)
    g = ((c + f32(1.0)) / f32(2.0)) * f32(size - 1)
    f = np.floor(g)
    w0 = (f + f32(1.0)) - g
    w1 = g - f
    assert g.dtype == f32 and w0.dtype == f32 and w1.dtype == f32
    return np.clip(f, -1e9, 1e9).astype(np.int64), w0, w1


def corners(key, H, W, xyz, mn, mx):
    """The four corners of plane `key` at every sample, in the order (h0,w0), (h0,w1), (h1,w0), (h1,w1):
    -> ih, iw [4, M] int64, w [4, M] float32 (wh * ww, rounded to float32), ok [4, M] bool (inside the plane)."""
    ah, aw = AXES[key]
    h0, wh0, wh1 = _axis(xyz[:, ah], mn[ah], mx[ah], H)
    w0, ww0, ww1 = _axis(xyz[:, aw], mn[aw], mx[aw], W)
    ih = np.stack([h0, h0, h0 + 1, h0 + 1])
    iw = np.stack([w0, w0 + 1, w0, w0 + 1])
    w = np.stack([wh0 * ww0, wh0 * ww1, wh1 * ww0, wh1 * ww1])
    assert w.dtype == f32
    ok = (ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)
    return ih, iw, w, ok


def _plane_chw(p):
    p = np.asarray(p)
    return p[0] if p.ndim == 4 else p


def forward(planes, xyz, mn, mx, aggregation='concat'):
    """planes: {'xy', 'yz', 'zx'} of [1, C, H, W] (or [C, H, W]) float32 -> (value, A), float64."""
    xyz = np.asarray(xyz, f32)
    vals, mags = [], []
    for key in KEYS:
        p = _plane_chw(planes[key]).astype(np.float64)
        C, H, W = p.shape
        ih, iw, w, ok = corners(key, H, W, xyz, mn, mx)
        v = np.zeros((xyz.shape[0], C))
        a = np.zeros((xyz.shape[0], C))
        for n in range(4):
            hh, ww_ = np.clip(ih[n], 0, H - 1), np.clip(iw[n], 0, W - 1)
            term = p[:, hh, ww_].T * (w[n].astype(np.float64) * ok[n])[:, None]
            v += term
            a += np.abs(term)
        vals.append(v); mags.append(a)
    if aggregation == 'concat':
        return np.concatenate(vals, 1), np.concatenate(mags, 1)
    return (vals[0] + vals[1]) + vals[2], (mags[0] + mags[1]) + mags[2]


def backward(shapes, xyz, mn, mx, grad_out, aggregation='concat'):
    """shapes: {'xy': (C, H, W), ...}; grad_out [M, 3C] (concat) or [M, C] (sum)
    -> {key: (grad [C, H, W], A [C, H, W], n [H, W])}, float64 / int64."""
    xyz = np.asarray(xyz, f32)
    g_all = np.asarray(grad_out, np.float64)
    out = {}
    for s, key in enumerate(KEYS):
        C, H, W = shapes[key]
        g = g_all[:, s * C:(s + 1) * C] if aggregation == 'concat' else g_all
        ih, iw, w, ok = corners(key, H, W, xyz, mn, mx)
        grad = np.zeros((H * W, C)); A = np.zeros((H * W, C)); cnt = np.zeros(H * W, np.int64)
        for n in range(4):
            k = ok[n]
            flat = ih[n][k] * W + iw[n][k]
            term = g[k] * w[n][k].astype(np.float64)[:, None]
            np.add.at(grad, flat, term)
            np.add.at(A, flat, np.abs(term))
            np.add.at(cnt, flat, 1)
        out[key] = (grad.reshape(H, W, C).transpose(2, 0, 1), A.reshape(H, W, C).transpose(2, 0, 1), cnt.reshape(H, W))
    return out
