"""Float64 statement of `dvgo_vm_bwd_xyz` and `dvgo_vm_density_bwd_xyz` (csrc/vm_xyz.hip): the gradient of the vector-matrix
features ([M, 3R]) and of the vector-matrix density ([M]) with respect to the sample position.  Test infrastructure, CPU
only, numpy, built on tests/triplane_oracle.py (`_axis`, AXES) and tests/vm_oracle.py (LINE_AXIS); `gamma`, SLACK and TINY
are tests/brick_oracle.py's.

Inputs (float32, bit for bit).  The cell of a sample in a plane, its node on a line and the per-axis weights are INPUTS of
the derivative, not part of what is bounded (tests/raygrad_oracle.py says why: the derivative has a kink on every lattice
line, so a float64 recomputation of the cell answers for another cell wherever rounding moved the point across one).
`inputs32` takes them from triplane_oracle._axis, which restates tp_axis on dvgo_src_index operation for operation.

Per sample, plane / line s (rows along world axis ah, columns along aw, line along al) and component r, in float64 from
those float32 inputs, corners and nodes out of range dropped as the forward drops them (zero padding, no clamp):
    p  = sum_ij (wh_i ww_j) v_ij        l  = w0 v0 + w1 v1                  (wh_i ww_j: the float32 product, an input of p)
    dh = sum_ij sgn_i ww_j v_ij         dw = sum_ij sgn_j wh_i v_ij         dn = v1 - v0           (sgn_0 = -1, sgn_1 = +1)
    ref[ah] += s_h sum_r g_r l dh       ref[aw] += s_w sum_r g_r l dw       ref[al] += s_n sum_r g_r p dn
    mag: the same sums over the absolute values of every term
with s_h = (H - 1) / (max[ah] - min[ah]) and likewise s_w, s_n (float64 from the float32 box; 0 for an axis of size 1) and
g_r = grad_out[m, s R + r] for the features, grad_out[m] for the density.

Bound.  u = 2^-24, gamma(k) = k u / (1 - k u).  On the way from its inputs to the output one term of the kernel's arithmetic
(include/dvgo_hip.h, the VM position block) passes, along a plane axis (g l dh):
    2       the two roundings of the line chain l = fmaf(v, w, l) from 0;
    1       the product t = g * l;
    4       at most 4 roundings of the corner chain dh = fmaf(v, c, dh) from 0 (c = +-ww or +-wh: the sign is exact);
    R       at most R roundings of the component chain Ah = fmaf(t, dh, Ah) from 0;
    3       the subtraction max - min of the scale, its division ((float)(H - 1) is exact) and the product Ah * scale;
    2       the additions across the three planes, from 0.0f (the first, 0 + t, is exact),
and along the line axis (g p dn):
    1 + 4   the weight product wh * ww and the 4 roundings of the corner chain of p;
    1       the product u = g * p;
    1       the subtraction dn = v1 - v0;
    R, 3, 2 as above,
so k = R + 12 on either path, and
    |got - ref| <= gamma(R + 12 + SLACK) mag + tiny.
SLACK = 1 covers the float64 evaluation of ref.  Underflow (gradual; no flush-to-zero flag in the build): an operation whose
result is subnormal adds at most TINY = 2^-149 absolute, which the later factors scale; an addition or subtraction is exact
when its result is subnormal.  Per plane and axis, as in hash_raygrad_oracle.py, with LA, DH, DN, PV the magnitudes of l,
dh (or dw), dn and sum_ij |v_ij|:
    plane axis: tiny = TINY * (|s| * (sum_r (2 |g| DH + 4 |g| LA + DH) + R) + unscaled + 1)
    line axis:  tiny = TINY * (|s| * (sum_r (|g| DN (PV + 4) + DN) + R) + unscaled + 1)
(line chain: 2 TINY |g| DH |s|; corner chain: 4 TINY |g| LA |s|; the product t: TINY DH |s|; the component chain: R TINY
|s|; the scale's division: TINY times the unscaled magnitude; the final product: TINY.  Line axis: weight products TINY
|v_ij| each and the corner chain 4 TINY, times |g| DN |s|; the product u: TINY DN |s|; the rest alike.)  A plane whose scale
is 0 adds none: 0 times a finite number is exact.  No constant here was fitted to GPU output, and no output is left out.
Where mag == 0 -- every term dropped (more than one cell outside, a NaN coordinate), an axis of size 1 everywhere it
appears, all-zero values or gradients -- the output must be exactly 0.0.
"""
import numpy as np

import triplane_oracle as TO
import vm_oracle as VO
from brick_oracle import SLACK, TINY, gamma
from interp_oracle import fma32

f32 = np.float32
KEYS = TO.KEYS
# sign of corner n = 00, 01, 10, 11 (rows, columns) in d/dh and in d/dw
_SGN_H = (-1.0, -1.0, 1.0, 1.0)
_SGN_W = (-1.0, 1.0, -1.0, 1.0)


def _chw(p):
    p = np.asarray(p)
    return p[0] if p.ndim == 4 else p


def _rn(ln):
    ln = np.asarray(ln)
    return ln[0, :, :, 0] if ln.ndim == 4 else ln


class Inputs:
    """One plane / line pair s: h0, w0, n0 [M] int64 floors; wh, ww, wn [2, M] float32 weights of the lower / upper node"""

    def __init__(self, h0, w0, n0, wh, ww, wn):
        self.h0, self.w0, self.n0, self.wh, self.ww, self.wn = h0, w0, n0, wh, ww, wn


def inputs32(key, H, W, N, xyz, mn, mx):
    """The kernel's float32 cell, node and weights of every sample in plane / line `key`, restated (tp_setup, tp_axis)."""
    p = np.asarray(xyz, f32).reshape(-1, 3)
    ah, aw = TO.AXES[key]
    al = VO.LINE_AXIS[key]
    with np.errstate(all='ignore'):
        h0, wh0, wh1 = TO._axis(p[:, ah], mn[ah], mx[ah], H)
        w0, ww0, ww1 = TO._axis(p[:, aw], mn[aw], mx[aw], W)
        n0, wn0, wn1 = TO._axis(p[:, al], mn[al], mx[al], N)
    return Inputs(h0, w0, n0, np.stack([wh0, wh1]), np.stack([ww0, ww1]), np.stack([wn0, wn1]))


def _gather(p, ln, I):
    """p [R,H,W], ln [R,N] -> corner values v [4, M, R] with ok [4, M]; node values vn [2, M, R] with okn [2, M]"""
    R, H, W = p.shape
    N = ln.shape[1]
    v, ok = [], []
    for i in range(2):
        for j in range(2):
            ih, iw = I.h0 + i, I.w0 + j
            ok.append((ih >= 0) & (ih < H) & (iw >= 0) & (iw < W))
            v.append(p[:, np.clip(ih, 0, H - 1), np.clip(iw, 0, W - 1)].T)
    vn, okn = [], []
    for i in range(2):
        n = I.n0 + i
        okn.append((n >= 0) & (n < N))
        vn.append(ln[:, np.clip(n, 0, N - 1)].T)
    return np.stack(v), np.stack(ok), np.stack(vn), np.stack(okn)


def scales(key, H, W, N, mn, mx):
    """(s_h, s_w, s_n) float64 from the float32 box"""
    mn, mx = np.asarray(mn, f32).astype(np.float64), np.asarray(mx, f32).astype(np.float64)
    ah, aw = TO.AXES[key]
    al = VO.LINE_AXIS[key]
    return (H - 1) / (mx[ah] - mn[ah]), (W - 1) / (mx[aw] - mn[aw]), (N - 1) / (mx[al] - mn[al])


class Sums:
    def __init__(self, ref, mag, tiny, R):
        self.ref, self.mag, self.tiny, self.R = ref, mag, tiny, R

    def k(self):
        return self.R + 12

    def bound(self):
        return gamma(self.k() + SLACK) * self.mag + self.tiny


def _grad_of(grad_out, M, R, s):
    g = np.asarray(grad_out)
    return g.reshape(M, 3 * R)[:, s * R:(s + 1) * R] if g.ndim == 2 else np.broadcast_to(g.reshape(M, 1), (M, R))


def sums(planes, lines, grad_out, xyz, mn, mx, inputs=None):
    """-> Sums with ref, mag, tiny [M,3] float64.  planes {'xy','yz','zx'} of [1,R,H,W], lines likewise of [1,R,N,1];
    grad_out [M, 3R] (the feature entry) or [M] (the density entry); `inputs`: {key: Inputs} (None: inputs32)."""
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    M = xyz.shape[0]
    R = _chw(planes['xy']).shape[0]
    ref, mag, tiny = np.zeros((M, 3)), np.zeros((M, 3)), np.zeros((M, 3))
    for s, key in enumerate(KEYS):
        p, ln = _chw(planes[key]).astype(np.float64), _rn(lines[key]).astype(np.float64)
        _, H, W = p.shape
        N = ln.shape[1]
        I = inputs32(key, H, W, N, xyz, mn, mx) if inputs is None else inputs[key]
        v, ok, vn, okn = _gather(p, ln, I)
        g = _grad_of(grad_out, M, R, s).astype(np.float64)
        wh, ww, wn = (np.asarray(a, np.float64) for a in (I.wh, I.ww, I.wn))
        k32 = [(I.wh[i] * I.ww[j]).astype(np.float64) for i in range(2) for j in range(2)]     # the float32 product
        pv = pa = dh = dha = dw = dwa = vsum = 0.0
        with np.errstate(invalid='ignore'):
            for n in range(4):                           # (a dropped term is dropped whatever its weight: a NaN weight too)
                i, j = n >> 1, n & 1
                o, vv = ok[n][:, None], v[n]
                pv = pv + np.where(o, k32[n][:, None] * vv, 0.0); pa = pa + np.where(o, np.abs(k32[n][:, None] * vv), 0.0)
                dh = dh + np.where(o, _SGN_H[n] * ww[j][:, None] * vv, 0.0); dha = dha + np.where(o, np.abs(ww[j][:, None] * vv), 0.0)
                dw = dw + np.where(o, _SGN_W[n] * wh[i][:, None] * vv, 0.0); dwa = dwa + np.where(o, np.abs(wh[i][:, None] * vv), 0.0)
                vsum = vsum + np.where(o, np.abs(vv), 0.0)
            v0, v1 = np.where(okn[0][:, None], vn[0], 0.0), np.where(okn[1][:, None], vn[1], 0.0)
            t0, t1 = np.where(okn[0][:, None], wn[0][:, None] * vn[0], 0.0), np.where(okn[1][:, None], wn[1][:, None] * vn[1], 0.0)
        lv, la = t0 + t1, np.abs(t0) + np.abs(t1)
        dn, dna = v1 - v0, np.abs(v1) + np.abs(v0)
        ga = np.abs(g)
        sh, sw, sn = scales(key, H, W, N, mn, mx)
        ah, aw = TO.AXES[key]
        al = VO.LINE_AXIS[key]
        for axis, sc, val, m_, under in (
                (ah, sh, (g * lv * dh).sum(1), (ga * la * dha).sum(1), (2 * ga * dha + 4 * ga * la + dha).sum(1)),
                (aw, sw, (g * lv * dw).sum(1), (ga * la * dwa).sum(1), (2 * ga * dwa + 4 * ga * la + dwa).sum(1)),
                (al, sn, (g * pv * dn).sum(1), (ga * pa * dna).sum(1), (ga * dna * (vsum + 4) + dna).sum(1))):
            if sc == 0:
                continue
            ref[:, axis] += sc * val
            mag[:, axis] += abs(sc) * m_
            tiny[:, axis] += np.where(m_ > 0, TINY * (abs(sc) * (under + R) + m_ + 1.0), 0.0)
    return Sums(ref, mag, tiny, R)


def check(S, got, what='vm_bwd_xyz'):
    """got [M,3] float32.  Every output inside the bound, exact 0.0 where mag == 0.  -> worst err / bound"""
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
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.size} outside gamma(R + 12 + {SLACK}) mag; first (index, got, '
                             f'ref, err, bound): {rows}')
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.where(bound > 0, err / bound, 0.0)
    return float(r.max()) if r.size else 0.0


def evaluate32(planes, lines, grad_out, xyz, mn, mx, drop_corner=None, flip=None, no_scale=False, clamp=False):
    """The kernel's float32 arithmetic in the stated order, in numpy (fmaf by interp_oracle.fma32) -> [M,3] float32.  The
    keyword arguments plant the mistakes tests/test_vm_raygrad_host.py expects the oracle to catch: a corner left out of
    dh and dw, the sign of dn flipped (`flip='n'`) or dh and dw swapped (`flip='hw'`), the scale left out, the derivative
    zeroed outside the box (an `inside` predicate the forward does not have)."""
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    mn, mx = np.asarray(mn, f32), np.asarray(mx, f32)
    M = xyz.shape[0]
    R = _chw(planes['xy']).shape[0]
    out = np.zeros((M, 3), f32)
    zero = np.zeros(M, f32)
    with np.errstate(all='ignore'):
        for s, key in enumerate(KEYS):
            p, ln = _chw(planes[key]).astype(f32), _rn(lines[key]).astype(f32)
            _, H, W = p.shape
            N = ln.shape[1]
            I = inputs32(key, H, W, N, xyz, mn, mx)
            v, ok, vn, okn = _gather(p, ln, I)
            g = _grad_of(grad_out, M, R, s).astype(f32)
            k = [(I.wh[i] * I.ww[j]).astype(f32) for i in range(2) for j in range(2)]
            ch = [-I.ww[0], -I.ww[1], I.ww[0], I.ww[1]]
            cw = [-I.wh[0], I.wh[0], -I.wh[1], I.wh[1]]
            if flip == 'hw':
                ch, cw = cw, ch
            Ah, Aw, An = zero.copy(), zero.copy(), zero.copy()
            for r in range(R):
                pv, dh, dw, l = zero.copy(), zero.copy(), zero.copy(), zero.copy()
                for n in range(4):
                    pv = np.where(ok[n], fma32(v[n][:, r], k[n], pv), pv)
                for n in range(2):
                    l = np.where(okn[n], fma32(vn[n][:, r], I.wn[n], l), l)
                for n in range(4):
                    if n == drop_corner:
                        continue
                    dh = np.where(ok[n], fma32(v[n][:, r], ch[n], dh), dh)
                    dw = np.where(ok[n], fma32(v[n][:, r], cw[n], dw), dw)
                dn = (np.where(okn[1], vn[1][:, r], f32(0)) - np.where(okn[0], vn[0][:, r], f32(0))).astype(f32)
                if flip == 'n':
                    dn = -dn
                t, u = (g[:, r] * l).astype(f32), (g[:, r] * pv).astype(f32)
                Ah, Aw, An = fma32(t, dh, Ah), fma32(t, dw, Aw), fma32(u, dn, An)
            ah, aw = TO.AXES[key]
            al = VO.LINE_AXIS[key]
            for axis, A, size in ((ah, Ah, H), (aw, Aw, W), (al, An, N)):
                sc = f32(1.0) if no_scale else f32(size - 1) / (mx[axis] - mn[axis])
                t = (A * sc).astype(f32)
                if clamp:
                    t = np.where((xyz[:, axis] >= mn[axis]) & (xyz[:, axis] <= mx[axis]), t, f32(0))
                out[:, axis] = out[:, axis] + t
    return out


def forward64(planes, lines, xyz, mn, mx, density=False):
    """The samplers in pure float64 (cell and weights too): [M, 3R], or their sum over the 3R products [M] (`density`).
    What the central differences of tests/test_vm_raygrad_host.py differentiate."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    mn, mx = np.asarray(mn, f32).astype(np.float64), np.asarray(mx, f32).astype(np.float64)
    out = []
    for key in KEYS:
        p, ln = _chw(planes[key]).astype(np.float64), _rn(lines[key]).astype(np.float64)
        R, H, W = p.shape
        N = ln.shape[1]
        ah, aw = TO.AXES[key]
        al = VO.LINE_AXIS[key]

        def axis(a, size):
            g = (xyz[:, a] - mn[a]) / (mx[a] - mn[a]) * (size - 1)
            f = np.floor(g)
            return f.astype(np.int64), np.stack([(f + 1) - g, g - f])
        h0, wh = axis(ah, H)
        w0, ww = axis(aw, W)
        n0, wn = axis(al, N)
        pv = np.zeros((xyz.shape[0], R))
        for i in range(2):
            for j in range(2):
                ih, iw = h0 + i, w0 + j
                ok = (ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)
                pv += p[:, np.clip(ih, 0, H - 1), np.clip(iw, 0, W - 1)].T * (wh[i] * ww[j] * ok)[:, None]
        lv = np.zeros((xyz.shape[0], R))
        for i in range(2):
            n = n0 + i
            ok = (n >= 0) & (n < N)
            lv += ln[:, np.clip(n, 0, N - 1)].T * (wn[i] * ok)[:, None]
        out.append(pv * lv)
    out = np.concatenate(out, 1)
    return out.sum(1) if density else out


# ------------------------------------------------------------------------------------------ inputs of the tests
import vm_density_cases as DC  # noqa: E402

MN, MX = DC.MN, DC.MX
# name -> (plane sizes, line lengths): non-square planes; one case with H = 1 and one with N = 1
SHAPES = {
    'base': (DC.SIZES, {'xy': 7, 'yz': 4, 'zx': 9}),
    'H1': ({'xy': (1, 7), 'yz': (6, 4), 'zx': (3, 9)}, {'xy': 7, 'yz': 4, 'zx': 9}),
    'N1': (DC.SIZES, DC.LINES),
}
RS = (1, 4, 5, 16)
MS = (1, 63, 64, 65, 1000)


def points(M, rng):
    """vm_density_cases.points (random points up to 30 % of the box outside it -- a cell of these planes is 11 % to 50 % of
    the box, so both less and more than one cell outside; the box corners and faces, lattice nodes of every plane and line,
    points several cells outside) with, from M = 63 on, one row with one NaN coordinate and one with three."""
    xyz = DC.points(M, rng)
    if M >= 63:
        xyz[44, 1] = np.nan
        xyz[45] = np.nan
    return xyz


def tensors(shape, R, rng):
    sizes, lens = SHAPES[shape]
    planes = {k: rng.standard_normal((1, R, *hw)).astype(f32) for k, hw in sizes.items()}
    lines = {k: rng.standard_normal((1, R, n, 1)).astype(f32) for k, n in lens.items()}
    return planes, lines


def in_box(xyz):
    """[M] bool: inside the closed box on every axis (False for a NaN)"""
    with np.errstate(invalid='ignore'):
        return np.all((xyz >= MN) & (xyz <= MX), axis=1)
