"""Oracle of the hash-grid sampler (csrc/hashgrid.hip; include/dvgo_hip.h, the hash block), numpy.

Coordinates, floors and weights in float32, operation for operation what the kernels do: the coordinate is
tests/triplane_oracle.py's `_axis` expression, then clamped into the lattice; where the clamp is idle `_axis` itself is
asserted to give the same floor and the same weight bits.  Rows in exact integer arithmetic (uint64 products masked to 32
bits); values and sums in float64.  Per sample m, level l, corner n (x slowest, z fastest) and channel c:
    w_n = (wx * wy) * wz (float32)          out[m, l F + c] = sum_n w_n * table[offsets[l] + row_n, c]

forward  -> value [M, L F] and A = sum |w v| per output.
backward -> per table element: grad = sum w g, A = sum |w g|, and per table row the count n of contributions.
"""
import numpy as np

import triplane_oracle as TO
from brick_oracle import SLACK, TINY, gamma

U = TO.U
f32 = np.float32
PRIMES = (1, 2654435761, 805459861)
M32 = (1 << 32) - 1


def axis(p, mn, mx, R):
    """float32: the floor node (int64, in [0, R - 2]) and the two weights of one axis of a level with R nodes."""
    p, mn, mx = np.asarray(p, f32), f32(mn), f32(mx)
    u = (p - mn) / (mx - mn)
    c = u * f32(2.0) - f32(1.0)
    g0 = ((c + f32(1.0)) / f32(2.0)) * f32(R - 1)
    g = np.minimum(np.maximum(g0, f32(0.0)), f32(R - 1))
    f = np.minimum(np.floor(g).astype(np.int64), R - 2)
    ff = f.astype(f32)
    w0 = (ff + f32(1.0)) - g
    w1 = g - ff
    assert g.dtype == f32 and w0.dtype == f32 and w1.dtype == f32
    idle = (g0 >= 0) & (g0 < f32(R - 1))                     # neither clamp acts: the library's one expression, as it stands
    tf, tw0, tw1 = TO._axis(p, mn, mx, R)
    assert (tf[idle] == f[idle]).all() and (tw0[idle].view(np.int32) == w0[idle].view(np.int32)).all() and \
        (tw1[idle].view(np.int32) == w1[idle].view(np.int32)).all()
    return f, w0, w1


def level_size(res, offsets, l):
    """(size_l, hashed): raises ValueError on a size that is neither the node count nor a power of two below it."""
    nodes = int(res[l][0]) * int(res[l][1]) * int(res[l][2])
    size = int(offsets[l + 1]) - int(offsets[l])
    if min(int(v) for v in res[l]) < 2:
        raise ValueError('a node count below 2')
    if size == nodes:
        return size, False
    if size < 1 or size > nodes or size & (size - 1):
        raise ValueError(f'level {l}: {size} rows for {nodes} nodes')
    return size, True


def node_rows(res, offsets, l, ix, iy, iz):
    """Rows (within the level) of the nodes (ix, iy, iz), int64 arrays of one shape."""
    size, hashed = level_size(res, offsets, l)
    ix, iy, iz = (np.asarray(v, np.int64) for v in (ix, iy, iz))
    if not hashed:
        return (ix * int(res[l][1]) + iy) * int(res[l][2]) + iz
    h = np.zeros(ix.shape, np.uint64)
    for v, prime in zip((ix, iy, iz), PRIMES):
        h ^= (v.astype(np.uint64) * np.uint64(prime)) & np.uint64(M32)          # (indices < 2^31, primes < 2^32: exact in uint64)
    return (h & np.uint64(size - 1)).astype(np.int64)


def corners(res, offsets, l, xyz, mn, mx):
    """The eight corners of level l at every sample -> rows [8, M] int64 (table rows, the level's offset included),
    w [8, M] float32, cell [M, 3] int64."""
    fw = [axis(xyz[:, a], mn[a], mx[a], int(res[l][a])) for a in range(3)]
    rows, w = [], []
    for n in range(8):
        b = ((n >> 2) & 1, (n >> 1) & 1, n & 1)
        rows.append(int(offsets[l]) + node_rows(res, offsets, l, *[fw[a][0] + b[a] for a in range(3)]))
        wn = (fw[0][1 + b[0]] * fw[1][1 + b[1]]) * fw[2][1 + b[2]]
        assert wn.dtype == f32
        w.append(wn)
    return np.stack(rows), np.stack(w), np.stack([fw[a][0] for a in range(3)], 1)


def forward(table, xyz, mn, mx, res, offsets):
    """table [T, F] float32 -> (value, A) [M, L F], float64."""
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    t = np.asarray(table).astype(np.float64)
    vals, mags = [], []
    for l in range(len(res)):
        rows, w, _ = corners(res, offsets, l, xyz, mn, mx)
        term = t[rows] * w.astype(np.float64)[:, :, None]                         # [8, M, F]
        vals.append(term.sum(0)); mags.append(np.abs(term).sum(0))
    return np.concatenate(vals, 1), np.concatenate(mags, 1)


def backward(shape, xyz, mn, mx, res, offsets, grad_out):
    """shape (T, F); grad_out [M, L F] -> (grad [T, F], A [T, F], n [T]), float64 / int64."""
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    T, F = shape
    g_all = np.asarray(grad_out, np.float64)
    grad = np.zeros((T, F)); A = np.zeros((T, F)); cnt = np.zeros(T, np.int64)
    for l in range(len(res)):
        rows, w, _ = corners(res, offsets, l, xyz, mn, mx)
        g = g_all[:, l * F:(l + 1) * F]
        for n in range(8):
            term = w[n].astype(np.float64)[:, None] * g
            np.add.at(grad, rows[n], term)
            np.add.at(A, rows[n], np.abs(term))
            np.add.at(cnt, rows[n], 1)
    return grad, A, cnt


def fwd_bound(A):
    """Two roundings in the weight and eight in the fma chain."""
    return gamma(10 + SLACK) * A + TINY


def bwd_bound(A, n, prefilled=0):
    """The weight (two roundings), the product, and n - 1 additions in any order (`prefilled`: 1 when the buffer held a
    value before, which is one more addition)."""
    return gamma(n[:, None] + 3 + prefilled + SLACK) * A + TINY


def same_cell_collisions(res, offsets, l, xyz, mn, mx):
    """How many samples have two of their eight corners of level l on one row."""
    rows, _, _ = corners(res, offsets, l, np.asarray(xyz, f32).reshape(-1, 3), mn, mx)
    srt = np.sort(rows, 0)
    return int((srt[1:] == srt[:-1]).any(0).sum())


def dense_expansion(table, res, offsets, l):
    """Level l as a dense array [Rx, Ry, Rz, F] float64, every node looked up."""
    Rx, Ry, Rz = (int(v) for v in res[l])
    ix, iy, iz = np.meshgrid(np.arange(Rx), np.arange(Ry), np.arange(Rz), indexing='ij')
    return np.asarray(table).astype(np.float64)[int(offsets[l]) + node_rows(res, offsets, l, ix, iy, iz)]


def brute_force(table, xyz, mn, mx, res, offsets):
    """Float64 throughout: every level expanded to a dense array, then plain trilinear interpolation with the coordinate
    clamped into the lattice.  -> [M, L F]."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    mn, mx = np.asarray(mn, np.float64), np.asarray(mx, np.float64)
    out = []
    for l in range(len(res)):
        D = dense_expansion(table, res, offsets, l)
        R = np.array([int(v) for v in res[l]], np.float64)
        g = np.clip((xyz - mn) / (mx - mn) * (R - 1), 0, R - 1)
        f = np.minimum(np.floor(g), R - 2).astype(np.int64)
        t = g - f
        acc = np.zeros((xyz.shape[0], D.shape[-1]))
        for n in range(8):
            b = np.array([(n >> 2) & 1, (n >> 1) & 1, n & 1])
            wgt = np.prod(np.where(b == 1, t, 1 - t), 1)
            acc += wgt[:, None] * D[f[:, 0] + b[0], f[:, 1] + b[1], f[:, 2] + b[2]]
        out.append(acc)
    return np.concatenate(out, 1)
