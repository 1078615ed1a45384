"""Oracle of the bilinear plane decoder's kernels (csrc/plane_rows.hip; lib/tri_dvgo.py:568-607 interpolate), numpy.

One MLP input row per sample and plane: [feat (C) | q0, q1 | sin (2P) | cos (2P) | cell_a, cell_b with cell_decode].

    plane   rows follow   columns follow   table (Ta rows, Tb columns)   cell
    xy      y             z                (Wx, Wy)                      (1 / Wx, 1 / Wy)
    yz      x             y                (Wy, Wz)                      (1 / Wy, 1 / Wz)
    zx      z             x                (Wz, Wx)                      (1 / Wz, 1 / Wx)

`rows(..., np.float32)` is what dvgo_plane_rows_fwd writes: feat, q and cell bit for bit -- the corner indices and weights
are triplane_oracle's float32 numbers, the four-corner chain acc = fmaf(v, w, acc) from 0 is evaluated with a correctly
rounded float32 fma (`fma32`), out-of-range corners skipped -- and the encoding columns as the float32 rounding of the
float64 sin / cos of the float32 argument q * 2^j (exact), to be compared within `ENC_ULPS`.
`rows(..., np.float64)` keeps the same float32 corner weights and q but sums the features in float64 in triplane_oracle's
order and leaves sin / cos in float64.  Bit-equality with triplane_oracle.forward's 'concat' value is carried by THIS
variant only: that oracle is a float64 sum, so the float32 rows' feat columns cannot equal it to the bit and are held to
(4 + 1) u A of it instead, the bound of a four-term fma chain -- not drift.  The float32 rows are what the kernel and
dvgo_triplane_fwd's own output are compared with bit for bit, on the GPU.
`scatter` is the float64 sum of the rows' gradient into the planes: triplane_oracle.backward on the feature columns.
`decode` strings rows -> MLPs -> aggregation together in torch float64, differentiable in the planes and the MLPs.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import triplane_oracle as TO  # noqa: E402

KEYS = TO.KEYS
TABLE = {'xy': (0, 1), 'yz': (1, 2), 'zx': (2, 0)}     # index into world_size of Ta (rows), of Tb (columns)
NET_OF = {'xy': 'xy', 'yz': 'yz', 'zx': 'yz'}          # the reference's self.interp['zx'] = self.interp_yz
U = 2.0 ** -24
# sinf / cosf of an exact argument: tests/posenc_oracle.py allows the position features 4 u of their value
ENC_ULPS = 4
f32 = np.float32


def fma32(a, b, c):
    """Correctly rounded float32 a * b + c.  The product of two float32 is exact in float64; the float64 sum is brought
    to round-to-odd with the exact error of the addition (TwoSum), after which the rounding to float32 is the rounding of
    the exact value (53 >= 24 + 2 bits)."""
    a, b, c = (np.asarray(v, f32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    odd = np.where(e > 0, np.nextafter(s, np.inf), np.nextafter(s, -np.inf))
    s = np.where((e != 0) & even & np.isfinite(s), odd, s)
    return s.astype(f32)


def node(i, T):
    """node_T(i) = i * (2 / (T - 1)) - 1 in float32; node_1 = -1."""
    step = f32(2) / f32(T - 1) if T > 1 else f32(0)
    return i.astype(f32) * step - f32(1)


def _chain32(vals, w, ok):
    acc = np.zeros(np.broadcast(vals[0], w[0]).shape, f32)
    for n in range(4):
        acc = np.where(ok[n], fma32(vals[n], w[n], acc), acc)
    return acc


def _chw(p):
    p = np.asarray(p)
    return p[0] if p.ndim == 4 else p


def feat(plane, key, xyz, mn, mx, dtype=f32):
    """The bilinear sample of one plane, [M, C]: float32 chain (the kernel's bits) or triplane_oracle's float64 sum."""
    p = _chw(plane).astype(f32)
    C, H, W = p.shape
    ih, iw, w, ok = TO.corners(key, H, W, xyz, mn, mx)
    vals = [p[:, np.clip(ih[n], 0, H - 1), np.clip(iw[n], 0, W - 1)].T for n in range(4)]
    if dtype == f32:
        return _chain32(vals, [w[n][:, None] for n in range(4)], [ok[n][:, None] for n in range(4)])
    v = np.zeros((xyz.shape[0], C))
    for n in range(4):
        v += vals[n].astype(np.float64) * (w[n].astype(np.float64) * ok[n])[:, None]
    return v


def coord(key, xyz, mn, mx, world_size):
    """(q0, q1) float32 [M]: the bilinear sample of the table that holds node_Tb(column) and node_Ta(row)."""
    ia, ib = TABLE[key]
    Ta, Tb = int(world_size[ia]), int(world_size[ib])
    ih, iw, w, ok = TO.corners(key, Ta, Tb, xyz, mn, mx)
    q0 = _chain32([node(iw[n], Tb) for n in range(4)], w, ok)
    q1 = _chain32([node(ih[n], Ta) for n in range(4)], w, ok)
    return q0, q1


def columns(C, P, cell_decode=True):
    """-> dict of slices into a row: feat, q, sin, cos, cell (empty without cell_decode); and D."""
    D = C + 2 + 4 * P + (2 if cell_decode else 0)
    return {'feat': slice(0, C), 'q': slice(C, C + 2), 'sin': slice(C + 2, C + 2 + 2 * P),
            'cos': slice(C + 2 + 2 * P, C + 2 + 4 * P), 'cell': slice(C + 2 + 4 * P, D)}, D


def tail(key, xyz, mn, mx, world_size, P, cell_decode=True, dtype=f32):
    """The row behind its features, [M, 2 + 4P (+ 2)]: q in float32; sin / cos of the float32 argument in float64, rounded
    to `dtype`; cells in float32."""
    q0, q1 = coord(key, xyz, mn, mx, world_size)
    q = np.stack([q0, q1], 1)
    arg = (q[:, :, None] * (f32(2) ** np.arange(P, dtype=f32))).reshape(len(q), 2 * P)       # k-major, exact
    assert arg.dtype == f32
    parts = [q.astype(dtype), np.sin(arg.astype(np.float64)).astype(dtype), np.cos(arg.astype(np.float64)).astype(dtype)]
    if cell_decode:
        ia, ib = TABLE[key]
        cell = np.array([f32(1) / f32(int(world_size[ia])), f32(1) / f32(int(world_size[ib]))], f32)
        parts.append(np.broadcast_to(cell, (len(q), 2)).astype(dtype))
    return np.concatenate(parts, 1)


def rows(planes, xyz, mn, mx, world_size, P, cell_decode=True, dtype=f32):
    """-> inp [3, M, D] of `dtype`: what dvgo_plane_rows_fwd writes (see the module docstring for what is exact)."""
    xyz = np.asarray(xyz, f32)
    out = []
    for key in KEYS:
        out.append(np.concatenate([feat(planes[key], key, xyz, mn, mx, dtype).astype(dtype),
                                   tail(key, xyz, mn, mx, world_size, P, cell_decode, dtype)], 1))
    return np.stack(out)


def scatter(shapes, xyz, mn, mx, grad_inp):
    """shapes: {'xy': (C, H, W), ...}; grad_inp [3, M, D] -> {key: (grad [C, H, W], A [C, H, W], n [H, W])}: the sum of
    tests/triplane_oracle.py's backward, over the first C columns of each plane's rows."""
    C = shapes['xy'][0]
    g = np.concatenate([np.asarray(grad_inp)[s][:, :C] for s in range(3)], 1)
    return TO.backward(shapes, np.asarray(xyz, f32), mn, mx, g, 'concat')


def decode(planes, nets, xyz, mn, mx, world_size, P, cell_decode=True, aggregation='concat'):
    """torch, float64: planes {'xy', ...} of [1, C, H, W] tensors, nets {'xy', 'yz'} of float64 modules -> [M, 3C] or [M, C].
    Corner indices, weights, q and cells are the float32 oracle's."""
    import torch
    xyz = np.asarray(xyz, f32)
    outs = []
    for key in KEYS:
        p = planes[key]
        _, C, H, W = p.shape
        ih, iw, w, ok = TO.corners(key, H, W, xyz, mn, mx)
        f = 0
        for n in range(4):
            hh, ww = torch.from_numpy(np.clip(ih[n], 0, H - 1)), torch.from_numpy(np.clip(iw[n], 0, W - 1))
            f = f + p[0][:, hh, ww].T.double() * torch.from_numpy(w[n].astype(np.float64) * ok[n])[:, None]
        t = torch.from_numpy(tail(key, xyz, mn, mx, world_size, P, cell_decode, np.float64))
        outs.append(nets[NET_OF[key]](torch.cat([f, t], -1)))
    return torch.cat(outs, 1) if aggregation == 'concat' else (outs[0] + outs[1]) + outs[2]
