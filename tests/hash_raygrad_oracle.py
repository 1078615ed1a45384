"""Float64 statement of `dvgo_hash_bwd_xyz` (csrc/hash_xyz.hip): the gradient of the hash-grid features with respect to the
sample position.  Test infrastructure, CPU only, numpy, built on tests/hash_oracle.py (`axis`, `node_rows`, `corners`);
`gamma`, SLACK and TINY are tests/brick_oracle.py's.

Inputs (float32, bit for bit).  The cell of a sample on a level, its per-axis weights and the predicate `inside` are INPUTS
of the derivative, not part of what is bounded (tests/raygrad_oracle.py says why: the derivative has a kink on every lattice
plane, so a float64 recomputation of the cell answers for another cell wherever rounding moved the point across a plane).
`inputs32` restates them in numpy float32 as csrc/hash_common.h does (`hash_axis`, `hash_inside`) and holds floor node and
weights to `hash_oracle.axis`'s bits.

Per sample, level l and axis a (x shown; d/dy pairs (wx, wz), d/dz pairs (wx, wy)), in float64 from those float32 inputs:
    s_l   = (Rx_l - 1) / (max[0] - min[0])                      (float64 from the float32 box)
    ref   = sum_l inside_lx * s_l * sum_c g[l F + c] sum_n sgn_n (wy_n wz_n) v_nc
    mag   = sum_l inside_lx * |s_l| * sum_c |g[l F + c]| sum_n |wy_n wz_n v_nc|
with sgn_n = -1 on the lower corner of the axis and +1 on the upper, g = grad_out, v_nc = table[row_n, c] (two corners of a
cell that share a row of a hashed level are two terms).

Bound.  u = 2^-24, gamma(k) = k u / (1 - k u).  On the way from its inputs to the output one term g (wy wz) v of the kernel's
arithmetic (include/dvgo_hip.h, the hash block) passes
    1       the product of the two weights (the sign is exact);
    8       at most 8 roundings of the corner chain d = fmaf(v, w2, d) from 0;
    F       at most F roundings of the channel chain a = fmaf(g_c, d_c, a) from 0;
    3       the subtraction max - min of the scale, its division ((float)(R - 1) is exact) and the product a * scale;
    L - 1   the additions across levels, ascending from 0.0f (the first, 0 + t, is exact; the select that drops a clamped
            axis is exact),
so k = F + L + 11 and
    |got - ref| <= gamma(F + L + 11 + SLACK) mag + tiny.
SLACK = 1 covers the float64 evaluation of ref.  Underflow (gradual; no flush-to-zero flag in the build): an operation whose
result is subnormal adds at most TINY = 2^-149 absolute, which the later factors scale; per level, as in raygrad_oracle.py,
    tiny_l = TINY * (|s_l| * (sum_c |g_c| * (sum_n |v_nc| + 8) + F) + unscaled_l + 1)
(weight product: TINY |v| |g| |s| per corner; corner chain: 8 TINY |g| |s|; channel chain: F TINY |s|; the scale's division:
TINY times the level's unscaled magnitude; the final product: TINY), summed over the levels that are inside on the axis; a
float32 addition is exact when its result is subnormal, so the level sum adds none.  No constant here was fitted to GPU
output, and no record is left out.  Where mag == 0 -- every level clamped on the axis, a NaN position, all-zero values or
gradients -- the output must be exactly 0.0.
"""
import numpy as np

import hash_oracle as HO
from brick_oracle import SLACK, TINY, gamma

f32 = np.float32
_BITS = np.array([[(n >> 2) & 1, (n >> 1) & 1, n & 1] for n in range(8)])
# the two axes whose weights multiply for the derivative along axis a, in the kernel's order (first * second)
_PAIR = {0: (1, 2), 1: (0, 2), 2: (0, 1)}


class Inputs:
    """One level: f [M,3] int64 floor nodes; w [M,3,2] float32 weight of the lower / upper node per axis; inside [M,3] bool"""

    def __init__(self, f, w, inside):
        self.f, self.w, self.inside = f, w, inside


def inputs32(xyz, mn, mx, res, l):
    """The kernel's float32 cell, per-axis weights and `inside` of every sample on level l, restated."""
    p = np.asarray(xyz, f32).reshape(-1, 3)
    mn, mx = np.asarray(mn, f32), np.asarray(mx, f32)
    fs, ws, ins = [], [], []
    for a in range(3):
        R = int(res[l][a])
        with np.errstate(all='ignore'):
            u = (p[:, a] - mn[a]) / (mx[a] - mn[a])
            c = u * f32(2.0) - f32(1.0)
            g0 = ((c + f32(1.0)) / f32(2.0)) * f32(R - 1)
            inside = (g0 >= f32(0.0)) & (g0 <= f32(R - 1))                 # (False for a NaN)
            g = np.fmin(np.fmax(g0, f32(0.0)), f32(R - 1))                 # fmaxf(NaN, 0) = 0, as on the device
            f = np.minimum(np.floor(g).astype(np.int64), R - 2)
            ff = f.astype(f32)
            w = np.stack([(ff + f32(1.0)) - g, g - ff], -1)
        assert w.dtype == f32 and g0.dtype == f32
        ok = ~np.isnan(p[:, a])                                             # (hash_oracle.axis clamps a NaN to NaN: not compared)
        hf, hw0, hw1 = HO.axis(p[ok, a], mn[a], mx[a], R)
        assert np.array_equal(hf, f[ok]) and np.array_equal(hw0.view(np.int32), w[ok, 0].view(np.int32)) and \
            np.array_equal(hw1.view(np.int32), w[ok, 1].view(np.int32))
        fs.append(f); ws.append(w); ins.append(inside)
    return Inputs(np.stack(fs, 1), np.stack(ws, 1), np.stack(ins, 1))


def scale(mn, mx, res, l):
    """s_l [3] float64 from the float32 box"""
    mn, mx = np.asarray(mn, f32).astype(np.float64), np.asarray(mx, f32).astype(np.float64)
    return (np.asarray(res[l], np.float64) - 1) / (mx - mn)


def corner_values(table, res, offsets, l, I):
    """v [M,8,F] float64: the rows of the eight corners of every sample's cell on level l"""
    t = np.asarray(table).astype(np.float64)
    v = []
    for n in range(8):
        ijk = I.f + _BITS[n]
        v.append(t[int(offsets[l]) + HO.node_rows(res, offsets, l, ijk[:, 0], ijk[:, 1], ijk[:, 2])])
    return np.stack(v, 1)


class Sums:
    def __init__(self, ref, mag, tiny, F, L):
        self.ref, self.mag, self.tiny, self.F, self.L = ref, mag, tiny, F, L

    def bound(self):
        return gamma(self.F + self.L + 11 + SLACK) * self.mag + self.tiny


def sums(table, grad_out, xyz, mn, mx, res, offsets, inputs=None):
    """-> Sums with ref, mag, tiny [M,3] float64.  table [T,F], grad_out [M, L F]; `inputs`: one Inputs per level (None:
    inputs32 of every level)."""
    p = np.asarray(xyz, f32).reshape(-1, 3)
    M, L, F = p.shape[0], len(res), np.asarray(table).shape[1]
    g_all = np.asarray(grad_out).reshape(M, L * F).astype(np.float64)
    ref, mag, tiny = np.zeros((M, 3)), np.zeros((M, 3)), np.zeros((M, 3))
    for l in range(L):
        I = inputs32(p, mn, mx, res, l) if inputs is None else inputs[l]
        v = corner_values(table, res, offsets, l, I)                                    # [M,8,F]
        g = g_all[:, l * F:(l + 1) * F]
        w = np.asarray(I.w, np.float64)
        s = scale(mn, mx, res, l)
        per = (np.abs(g) * (np.abs(v).sum(1) + 8)).sum(-1) + F                          # [M]
        for a in range(3):
            q, r = _PAIR[a]
            lref, lmag = np.zeros(M), np.zeros(M)
            for n in range(8):
                w2 = w[:, q, _BITS[n][q]] * w[:, r, _BITS[n][r]]
                sgn = 1.0 if _BITS[n][a] else -1.0
                term = w2[:, None] * v[:, n]                                            # [M,F]
                lref += sgn * (g * term).sum(-1)
                lmag += (np.abs(g) * np.abs(term)).sum(-1)
            ins = I.inside[:, a]
            ref[:, a] += np.where(ins, lref * s[a], 0.0)
            mag[:, a] += np.where(ins, lmag * abs(s[a]), 0.0)
            tiny[:, a] += np.where(ins, TINY * (abs(s[a]) * per + lmag + 1.0), 0.0)
    return Sums(ref, mag, tiny, F, L)


def check(S, got, what='hash_bwd_xyz'):
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
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.size} outside gamma(F + L + 11 + {SLACK}) mag; first (index, got, '
                             f'ref, err, bound): {rows}')
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.where(bound > 0, err / bound, 0.0)
    return float(r.max()) if r.size else 0.0


def evaluate32(table, grad_out, xyz, mn, mx, res, offsets, drop_corner=None, flip_axis=None, no_scale=False, no_clamp=False):
    """The kernel's float32 arithmetic in the stated order, in numpy (fmaf by brick_oracle.fma32) -> [M,3] float32.  The
    keyword arguments plant the mistakes tests/test_hash_raygrad_host.py expects the oracle to catch."""
    from brick_oracle import fma32
    p = np.asarray(xyz, f32).reshape(-1, 3)
    mn, mx = np.asarray(mn, f32), np.asarray(mx, f32)
    table = np.asarray(table, f32)
    M, L, F = p.shape[0], len(res), table.shape[1]
    g_all = np.asarray(grad_out, f32).reshape(M, L * F)
    out = np.zeros((M, 3), f32)
    for l in range(L):
        I = inputs32(p, mn, mx, res, l)
        v = corner_values(table, res, offsets, l, I).astype(f32)
        for a in range(3):
            q, r = _PAIR[a]
            acc = np.zeros(M, f32)
            for c in range(F):
                d = np.zeros(M, f32)
                for n in range(8):
                    if n == drop_corner:
                        continue
                    w2 = (I.w[:, q, _BITS[n][q]] * I.w[:, r, _BITS[n][r]]).astype(f32)
                    sgn = 1.0 if _BITS[n][a] else -1.0
                    if flip_axis == a:
                        sgn = -sgn
                    d = fma32(v[:, n, c], f32(sgn) * w2, d)
                acc = fma32(g_all[:, l * F + c], d, acc)
            sc = f32(1.0) if no_scale else f32(int(res[l][a]) - 1) / (mx[a] - mn[a])
            t = (acc * sc).astype(f32)
            out[:, a] = out[:, a] + (t if no_clamp else np.where(I.inside[:, a], t, f32(0.0)))
    return out


# ------------------------------------------------------------------------------------------ inputs of the tests
MN = np.array([-0.5, -1.25, -0.25], f32)
MX = np.array([1.5, 2.75, 0.75], f32)


def _table(levels):
    """[(res, rows or None for dense)] -> res int32 [L,3], offsets int64 [L+1]"""
    res = np.array([r for r, _ in levels], np.int32)
    sizes = [int(np.prod(r)) if rows is None else rows for r, rows in levels]
    return res, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _shift(t, by):
    return t[0], t[1] + by


# name -> (res, offsets): the level tables of the GPU test
LEVEL_TABLES = {
    'one_2x2x2': _table([((2, 2, 2), None)]),                                     # the smallest lattice: every point in the last cell
    'dense_and_hashed': _table([((3, 5, 9), None), ((17, 9, 33), 256)]),
    'L5_mixed': _table([((2, 3, 2), None), ((5, 5, 5), 8), ((4, 9, 6), None), ((12, 7, 20), 64), ((33, 17, 9), 512)]),
    'L16': _table([((2 + l, 3 + 2 * l, 2 + 3 * l), None if l < 6 else 256) for l in range(16)]),
    'L32_small': _table([((2 + l % 3, 2 + l % 4, 2 + l % 5), None if l % 2 == 0 or (2 + l % 3) * (2 + l % 4) * (2 + l % 5) <= 4 else 4)
                         for l in range(32)]),
    'offset0': _shift(_table([((3, 4, 5), None), ((9, 9, 9), 32)]), 24),          # offsets[0] > 0
}
SAMPLE_COUNTS = [0, 1, 257]
N_FAMILIES = 10


def points(M, seed):
    """[M,3] float32 world positions by family (index mod 10), in units of the box (MN, MX) so that they mean the same on
    every level: 0-1 interior; 2 on an interior lattice plane of the 3- and 5-node levels on one axis (u = 1/2), 3 on all
    three; 4 on one of the six faces (g == 0 or g == R - 1: u is exactly 0 or 1); 5 outside on one axis, 6 on two, 7 on
    three; 8 one NaN coordinate row (all three NaN); 9 a box corner."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(0.02, 0.98, (M, 3))
    rows = np.arange(M)
    fam = rows % N_FAMILIES
    axis = rng.integers(0, 3, M)
    side = rng.integers(0, 2, M)
    one = np.zeros((M, 3), bool)
    one[rows, axis] = True
    two = ~np.roll(one, 1, 1)
    out = np.where(rng.integers(0, 2, (M, 3)) == 1, 1.0 + rng.uniform(0.05, 0.9, (M, 3)), -rng.uniform(0.05, 0.9, (M, 3)))
    u = np.where((fam == 2)[:, None] & one, 0.5, u)
    u = np.where((fam == 3)[:, None], 0.5, u)
    u = np.where((fam == 4)[:, None] & one, side[:, None].astype(np.float64), u)
    u = np.where((fam == 5)[:, None] & one, out, u)
    u = np.where((fam == 6)[:, None] & two, out, u)
    u = np.where((fam == 7)[:, None], out, u)
    u = np.where((fam == 9)[:, None], rng.integers(0, 2, (M, 3)).astype(np.float64), u)
    mn, mx = MN.astype(np.float64), MX.astype(np.float64)
    p = (mn + u * (mx - mn)).astype(f32)
    p[fam == 8] = np.nan
    return p


def table_values(rows, F, seed):
    return np.random.default_rng(seed).standard_normal((rows, F)).astype(f32)


def grad_values(M, C, seed):
    return np.random.default_rng(seed).standard_normal((M, C)).astype(f32)
