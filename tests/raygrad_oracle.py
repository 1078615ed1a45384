"""Float64 statement of `dvgo_grid_sample_bwd_xyz` (csrc/grid_sample_xyz.hip): the gradient of the trilinear sample with
respect to the sample position.  Test infrastructure, CPU only, numpy.  `tri_setup`, `gamma`, SLACK and TINY are
tests/brick_oracle.py's (pinned to oracle/dvgo_oracle.c by tests/test_brick_oracle_host.py).

Inputs (float32, bit for bit).  The cell of a sample and its per-axis weights are INPUTS of the derivative, not part of what
is bounded: the derivative of a piecewise-trilinear function has a kink on every lattice plane, so a float64 recomputation of
the cell answers for a different cell wherever float32 rounding moved the point across a plane, and is wrong there by the
size of the kink, not by rounding.  `inputs32` restates them in numpy float32 as csrc/common.h does (`dvgo_src_index`,
`dvgo_tri_from_g`: floor corner ijk0, weights (f + 1) - g and g - f per axis); the floor corner, the in-range test and the
corners' voxels are `tri_setup`'s, and the restated weights are held to `tri_setup`'s corner weights bit for bit.

Per sample and axis a (x shown; y pairs (wz, wx), z pairs (wy, wx)), in float64 from those float32 inputs:
    s    = (X - 1) / (max[0] - min[0])                          (float64 from the float32 box)
    ref  = s * sum_c g_c sum_n sgn_n (wz_n wy_n) v_nc           over the corners n inside the lattice (zero padding)
    mag  = |s| * sum_c |g_c| sum_n |wz_n wy_n v_nc|
with sgn_n = -1 on the lower corner of the axis and +1 on the upper, g = grad_out, v the grid values.

Bound.  u = 2^-24, gamma(k) = k u / (1 - k u).  On the way from its inputs to the output, one term g_c (wz wy) v of the kernel's
arithmetic (include/dvgo_hip.h) passes
    1   the product of the two weights, wz * wy (the sign is exact);
    8   at most 8 roundings of the corner chain d = fmaf(v, w2, d) from 0 (a fused multiply-add rounds once; a term that
        enters at corner n = 0..7 passes 8 - n <= 8 of them);
    C   at most C roundings of the channel chain a = fmaf(g_c, d_c, a) from 0;
    1   the subtraction max - min of the scale, 1 its division ((float)(X - 1) is exact), 1 the final product a * scale,
so k = C + 12 and
    |got - ref| <= gamma(C + 12 + SLACK) mag + tiny.
SLACK = 1 covers the float64 evaluation of ref (a few 2^-53 mag).  Underflow (gradual: the build passes no flush-to-zero
flag): an operation whose result is subnormal adds at most TINY = 2^-149 absolute, which the later factors scale:
    tiny = TINY * (|s| * (sum_c |g_c| * (sum_n |v_nc| + 8) + C) + mag / |s| + 1)
(weight product: TINY |v| |g| |s| per corner; corner chain: 8 TINY |g| |s|; channel chain: C TINY |s|; the scale's division:
TINY times the unscaled sum; the final product: TINY).  No constant here was fitted to GPU output, and no record is left out.
Where mag == 0 -- every corner outside the lattice, an axis of size 1 (s = 0), all-zero values or gradients -- the output
must be exactly 0.0.
"""
import numpy as np

from brick_oracle import SLACK, TINY, gamma, tri_setup

_F = np.float32
# corner n: bit2 = +X, bit1 = +Y, bit0 = +Z (the gather's order)
_BITS = np.array([[(n >> 2) & 1, (n >> 1) & 1, n & 1] for n in range(8)])
# the two axes whose weights multiply for the derivative along axis a, in the kernel's order (first * second)
_PAIR = {0: (2, 1), 1: (2, 0), 2: (1, 0)}


class Inputs:
    """ijk0 [M,3] int64 floor corners; w [M,3,2]: weight of the lower / upper corner per axis; inb [M,8] bool"""

    def __init__(self, ijk0, w, inb):
        self.ijk0, self.w, self.inb = ijk0, w, inb


def inputs32(xyz, xyz_min, xyz_max, dims):
    """The kernel's float32 cell and per-axis weights of every sample, restated (see the module docstring)."""
    X, Y, Z = dims
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    mn, mx = np.asarray(xyz_min, np.float32), np.asarray(xyz_max, np.float32)
    ijk0, w8, inb, _ = tri_setup(p, mn, mx, X, Y, Z)
    size1 = np.array([X - 1, Y - 1, Z - 1], np.float32)
    with np.errstate(all='ignore'):
        u = (p - mn) / (mx - mn)
        c = u * _F(2.0) - _F(1.0)
        g = ((c + _F(1.0)) / _F(2.0)) * size1
    f = np.floor(g)
    w = np.stack([(f + _F(1.0)) - g, g - f], -1).astype(np.float32)
    assert np.array_equal(f.astype(np.int64), ijk0)
    for n in range(8):                                   # the restatement is tri_setup's, bit for bit
        bx, by, bz = _BITS[n]
        prod = (w[:, 2, bz] * w[:, 1, by]) * w[:, 0, bx]
        assert np.array_equal(prod.view(np.int32), w8[:, n].view(np.int32))
    return Inputs(ijk0, w, inb)


def inputs64(xyz, xyz_min, xyz_max, dims):
    """The same quantities evaluated in float64 from float64 positions (tests/test_raygrad_oracle_host.py: the formula
    against torch autograd, at points whose float32 and float64 cells agree)."""
    p = np.asarray(xyz, np.float64).reshape(-1, 3)
    mn, mx = np.asarray(xyz_min, np.float64), np.asarray(xyz_max, np.float64)
    g = (p - mn) / (mx - mn) * (np.asarray(dims, np.float64) - 1)
    f = np.floor(g)
    ijk0 = f.astype(np.int64)
    w = np.stack([(f + 1.0) - g, g - f], -1)
    inb = np.empty((p.shape[0], 8), bool)
    for n in range(8):
        ijk = ijk0 + _BITS[n]
        inb[:, n] = np.all((ijk >= 0) & (ijk < np.asarray(dims)), -1)
    return Inputs(ijk0, w, inb)


def scale(xyz_min, xyz_max, dims):
    """s [3] float64 from the float32 box"""
    mn, mx = np.asarray(xyz_min, np.float32).astype(np.float64), np.asarray(xyz_max, np.float32).astype(np.float64)
    return (np.asarray(dims, np.float64) - 1) / (mx - mn)


class Sums:
    def __init__(self, ref, mag, tiny, C):
        self.ref, self.mag, self.tiny, self.C = ref, mag, tiny, C

    def bound(self):
        return gamma(self.C + 12 + SLACK) * self.mag + self.tiny


def corner_values(grid, I):
    """grid [C,X,Y,Z] -> v [M,8,C] float64, 0 where the corner is outside"""
    grid = np.asarray(grid)
    C, X, Y, Z = grid.shape
    M = I.ijk0.shape[0]
    v = np.zeros((M, 8, C), np.float64)
    for n in range(8):
        ijk = I.ijk0 + _BITS[n]
        ok = I.inb[:, n]
        v[ok, n] = np.moveaxis(grid[:, ijk[ok, 0], ijk[ok, 1], ijk[ok, 2]], 0, -1)
    return v


def sums(grid, grad_out, I, s):
    """-> Sums with ref, mag, tiny [M,3] float64.  grid [C,X,Y,Z], grad_out [M,C], I: Inputs, s [3]."""
    v = corner_values(grid, I)
    M, _, C = v.shape
    g = np.asarray(grad_out).reshape(M, C).astype(np.float64)
    w = np.asarray(I.w, np.float64)
    s = np.asarray(s, np.float64)
    ref, mag = np.zeros((M, 3)), np.zeros((M, 3))
    for a in range(3):
        p, q = _PAIR[a]
        for n in range(8):
            w2 = w[:, p, _BITS[n][p]] * w[:, q, _BITS[n][q]]
            sgn = 1.0 if _BITS[n][a] else -1.0
            term = np.where(I.inb[:, n, None], w2[:, None] * v[:, n], 0.0)            # [M,C]
            ref[:, a] += sgn * (g * term).sum(-1)
            mag[:, a] += (np.abs(g) * np.abs(term)).sum(-1)
    unscaled = mag.copy()
    ref, mag = ref * s, mag * np.abs(s)
    vabs = (np.abs(v) * I.inb[:, :, None]).sum(1)                                     # [M,C]
    per = (np.abs(g) * (vabs + 8)).sum(-1) + C                                        # [M]
    tiny = TINY * (np.abs(s)[None, :] * per[:, None] + unscaled + 1.0)
    return Sums(ref, mag, tiny, C)


def check(S, got, what='grid_sample_bwd_xyz'):
    """got [M,3] float32.  Every record inside the bound, exact 0.0 where mag == 0.  -> worst err / bound"""
    got = np.asarray(got, np.float32).reshape(-1, 3).astype(np.float64)
    assert got.shape == S.ref.shape, (got.shape, S.ref.shape)
    if not np.all(np.isfinite(got)):
        idx = np.argwhere(~np.isfinite(got))[:5]
        raise AssertionError(f'{what}: {int((~np.isfinite(got)).sum())} non-finite (unwritten?) elements; first {idx.tolist()}')
    zero = S.mag == 0
    if np.any(zero & (got != 0)):
        idx = np.argwhere(zero & (got != 0))[:5]
        raise AssertionError(f'{what}: non-zero where nothing contributes; first {[(tuple(i), got[tuple(i)]) for i in idx]}')
    err = np.abs(got - S.ref)
    bound = np.where(zero, 0.0, S.bound())
    bad = err > bound
    if np.any(bad):
        idx = np.argwhere(bad)[:5]
        rows = [(tuple(int(k) for k in i), got[tuple(i)], S.ref[tuple(i)], err[tuple(i)], bound[tuple(i)]) for i in idx]
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.size} outside gamma(C + 12 + {SLACK}) mag; first (index, got, ref, err, bound): {rows}')
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.where(bound > 0, err / bound, 0.0)
    return float(r.max()) if r.size else 0.0


def evaluate32(grid, grad_out, I, xyz_min, xyz_max, dims, drop_corner=None, flip_axis=None, no_scale=False):
    """The kernel's float32 arithmetic in the stated order, in numpy (fmaf by brick_oracle.fma32) -> [M,3] float32.
    The keyword arguments plant the mistakes tests/test_raygrad_oracle_host.py expects the oracle to catch."""
    from brick_oracle import fma32
    grid = np.asarray(grid, np.float32)
    C = grid.shape[0]
    M = I.ijk0.shape[0]
    v = corner_values(grid, I).astype(np.float32)
    g = np.asarray(grad_out, np.float32).reshape(M, C)
    w = np.asarray(I.w, np.float32)
    mn, mx = np.asarray(xyz_min, np.float32), np.asarray(xyz_max, np.float32)
    out = np.zeros((M, 3), np.float32)
    for a in range(3):
        p, q = _PAIR[a]
        acc = np.zeros(M, np.float32)
        for c in range(C):
            d = np.zeros(M, np.float32)
            for n in range(8):
                if n == drop_corner:
                    continue
                w2 = (w[:, p, _BITS[n][p]] * w[:, q, _BITS[n][q]]).astype(np.float32)
                sgn = 1.0 if _BITS[n][a] else -1.0
                if flip_axis == a:
                    sgn = -sgn
                d = np.where(I.inb[:, n], fma32(v[:, n, c], _F(sgn) * w2, d), d).astype(np.float32)
            acc = fma32(g[:, c], d, acc)
        sc = _F(1.0) if no_scale else _F(dims[a] - 1) / (mx[a] - mn[a])
        out[:, a] = acc * sc
    return out


# ------------------------------------------------------------------------------------------ inputs of the tests
MN = np.array([-0.5, -1.25, -0.25], np.float32)
MX = np.array([1.5, 2.75, 0.75], np.float32)
# (C, layout, dims, float offset of the base): every dispatch branch of the kernel and the shapes that can go wrong
GRIDS = [(1, 'cf', (3, 4, 5), 0), (12, 'cl', (4, 3, 6), 0), (12, 'cl', (4, 3, 6), 1), (3, 'cl', (5, 5, 2), 0),
         (5, 'cf', (2, 6, 3), 0), (1, 'cf', (1, 4, 4), 0)]
SAMPLE_COUNTS = [0, 1, 257]


def points(dims, M, seed):
    """[M,3] float32 world positions in the box (MN, MX), by family (index mod 8): 0-1 interior; 2 on a lattice plane of
    one axis, 3 of all three (a node); 4 on one of the six faces; 5 up to one cell outside on one axis and 6 on all
    three (some corners padded); 7 more than one cell outside on one axis (every corner padded: exact zeros)."""
    rng = np.random.default_rng(seed)
    size1 = np.maximum(np.asarray(dims, np.float64) - 1, 1)          # (an axis of size 1 has one node, at any position)
    g = rng.uniform(0.02, 0.98, (M, 3)) * size1
    node = np.floor(rng.uniform(0, 1, (M, 3)) * (size1 + 1)).clip(0, size1)
    axis = rng.integers(0, 3, M)
    side = rng.integers(0, 2, M)
    rows = np.arange(M)
    fam = rows % 8
    one = np.zeros((M, 3), bool)
    one[rows, axis] = True
    g = np.where((fam == 2)[:, None] & one, node, g)
    g = np.where((fam == 3)[:, None], node, g)
    g = np.where((fam == 4)[:, None] & one, (side * size1[axis])[:, None], g)
    out1 = np.where(rng.integers(0, 2, (M, 3)) == 1, size1 + rng.uniform(0.05, 0.95, (M, 3)), -rng.uniform(0.05, 0.95, (M, 3)))
    g = np.where((fam == 5)[:, None] & one, out1, g)
    g = np.where((fam == 6)[:, None], out1, g)
    far = np.where(side == 1, size1[axis] + rng.uniform(1.2, 2.5, M), -rng.uniform(1.2, 2.5, M))
    g = np.where((fam == 7)[:, None] & one, far[:, None], g)
    mn, mx = MN.astype(np.float64), MX.astype(np.float64)
    return (mn + g / size1 * (mx - mn)).astype(np.float32)


def grid_values(C, dims, seed):
    return np.random.default_rng(seed).standard_normal((C, *dims)).astype(np.float32)


def grad_values(M, C, seed):
    return np.random.default_rng(seed).standard_normal((M, C)).astype(np.float32)
