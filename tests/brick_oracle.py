"""Float64 statement of the brick scatter and of the Adam update fused into it (test infrastructure, CPU only).

It takes what `dvgo_brick_accumulate` takes at the library boundary (include/dvgo_hip.h): the record list
{kept index or -1, ray, step, density gradient} with the per-brick list offsets, `rays_start`, `rays_dir`, `stepdist`,
the bounding box, `grad_feat`, C and the lattice; for the update also p, m, v of both grids before the launch, the two
step sizes, betas, eps and the two masked flags.

Inputs of the sum (float32, bit for bit).  Sample positions and trilinear weights are not part of what is bounded: they
are restated here in numpy float32 operation for operation as csrc/common.h does them -- `march_dist`, three `fmaf`
(`fma32`: the exact sum by TwoSum, rounded to odd in float64 and then to float32, which is a correctly rounded fused
multiply-add), `dvgo_src_index`, `dvgo_tri_from_g`, `dvgo_tri_inb`, `dvgo_tri_weight`.  tests/test_brick_oracle_host.py
pins that restatement against oracle/dvgo_oracle.c bit for bit.

Per voxel and channel, float64 (the density gradient rides as channel C, as in the kernel):
    ref = sum w g        mag = sum |w| |g|        n = number of contributions
over the corners of the listed records that lie inside the listing brick and inside the lattice (brick.hip:212-219), so
every corner is attributed once, to the brick that owns its voxel.  S = max(1, ceil(n_b / slice_len)) slices for a
brick of n_b entries when heavy-brick tables are in use, else 1.

Gradient bound.  u = 2^-24, gamma(k) = k u / (1 - k u) (Higham, Accuracy and Stability, Lemma 3.1).
  brick   every voxel is formed by n `fmaf(w, g, acc)` steps in some order (n roundings: the product is exact inside the
          fused operation) and at most S - 1 float additions where the slices meet; data parallel (modes 2 then 3) adds
          R - 1 additions of the R ranks' tiles.  |got - ref| <= gamma(n + S + R - 1 + SLACK) mag.
  atomic  `naive` rounds each product and adds it to memory: 1 + n roundings on a term's path.  `dedup` / `rows` first
          add the products of a wavefront pass in a table and then add each table entry to memory: a term of a table of
          k_t products passes its own product rounding, at most k_t additions in the table and at most T additions in
          memory (T tables); every other table holds at least one product, so k_t + T <= n + 1.
          |got - ref| <= gamma(n + 2 + SLACK) mag for all three.
  SLACK = 1 covers the oracle's own float64 summation (n 2^-53 mag < u mag for n < 2^29).  Nothing else is hidden in it.
  Underflow: an operation whose result is subnormal carries an absolute error of at most TINY = 2^-149 (gradual
  underflow; the build passes no flush-to-zero flag), (n + S) TINY per voxel.
Where mag == 0 (no contribution, or every term zero) the dense output must be exactly 0.0: every voxel of an untouched
brick, and the in-grid voxels of partial bricks on the upper faces.  No constant here was fitted to GPU output.

Adam (adam_upd_kernel.cu:25-40 = `adam_one` of common.h), `dg` the gradient bound above, b1, b2, eps, ss as float32:
    t = fl((1 - b1) g)                 m1 = fl(b1 m0 + t)            (fmaf: one rounding)
    s = fl((1 - b2) g), q = fl(s g)    v1 = fl(b2 v0 + q)
    a = fl(ss m1), r = fl(sqrt v1), d = fl(r + eps), st = fl(a / d),  p1 = fl(p0 - st)
1 - b1 and 1 - b2 are exact in float32 (Sterbenz: b in [0.5, 1]).  Each piece is checked on its own:
  m   g_m = (m1 - b1 m0) / (1 - b1).  m1 (1 + d) = b1 m0 + t gives |m1 - b1 m0 - t| <= u |m1|, and |t - (1 - b1) g| <=
      (1 - b1) u |g|, so |g_m - g| <= u |g| + u |m1| / (1 - b1): one u of |m1| over (1 - b1), one of |g|.
      Against ref: |g_m - ref| <= dg + u (|ref| + dg) + u |m1| / (1 - b1).
  v   g_v2 = (v1 - b2 v0) / (1 - b2).  q carries two roundings, v1 one: |g_v2 - g^2| <= (2u + u^2) g^2 +
      u |v1| / (1 - b2), and |g^2 - ref^2| <= dg (2 |ref| + dg).  The check is made on the squares: it is the statement
      "carried through the square root" multiplied by (|g_v| + |ref|), without a division by a sum that may vanish.
  p   p1 against p0 - ss m1 / (sqrt(v1) + eps) evaluated in float64 FROM THE DEVICE'S OWN m1, v1: the step is four
      float32 operations (product, square root, sum, quotient; square root and division are correctly rounded -- the
      compiler's default for HIP, and build.py passes no flag that relaxes it), the subtraction a fifth whose error is
      relative to p1: |p1 - (p0 - step)| <= gamma(4) |step| + u (|p0| + (1 + gamma(4)) |step|).  Cancellation in the
      gradient never enters: a parameter is held to a few ulp of |p0| + |step| whatever its gradient was.
  Every u above is taken as 1.01 u (second-order terms and the float64 evaluation of the recovery, itself bounded by
  2^-50 (|m0| or |v0|) / (1 - b)); each rounding also gets TINY for underflow.
Since m, v and p are each tied to the same `ref` (m and v) or to the device's own m1, v1 (p), an element whose three
values came from different gradients or different rules fails one of the three.

Masked rule, per element (adam_upd_kernel.cu:35: skip iff the gradient is exactly 0):
    mag == 0           p, m, v bit-identical to before
    |ref| > dg         updated: all three checks above hold
    0 < |ref| <= dg    undetermined (the float32 sum may or may not have cancelled to 0): either all three are
                       bit-identical to before, or all three pass as updated -- never a mixture
Undetermined elements may be at most MAX_UNDETERMINED = 1e-4 of the elements with mag > 0.
Unmasked (unreachable from TrainStep, `can_fuse_grid_step`; documented meaning): plain Adam with the summed gradient,
0 included, on every in-grid voxel of a LISTED brick (n_b > 0); nothing elsewhere.

`LaunchSpy` wraps `directvoxgo_amd._lib.call`: for every `dvgo_brick_accumulate` it keeps the arguments and clones of
the records and of p, m, v before the launch and holds the result to this oracle after it, so the oracle always runs on
the kernel's actual inputs -- in any scene, inside TrainStep, including the density gradient that rides in the records.
"""
import contextlib

import numpy as np

U = 2.0 ** -24
SLACK = 1
TINY = 2.0 ** -149
MAX_UNDETERMINED = 1e-4
BRICK = 8
_F = np.float32


def gamma(k):
    k = np.asarray(k, np.float64)
    return k * U / (1.0 - k * U)


# ------------------------------------------------------------------------------------------ float32 restatement
def fma32(a, b, c):
    """Correctly rounded float32 fma: a * b is exact in float64, TwoSum gives the exact sum, which is rounded to odd in
    float64 (29 guard bits over float32) and then to float32."""
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64) if s.ndim else np.array(s).view(np.int64)
    even = (bits & 1) == 0
    nudged = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    odd = np.where((err != 0) & even, nudged, s)
    return odd.astype(np.float32)


def march_dist(stepdist, step):
    sd = _F(stepdist)
    step = np.asarray(step).astype(np.float32)
    return sd * step if sd > 0 else step / (-sd)


def positions(recs, rays_start, rays_dir, stepdist):
    """[E, 3] float32 sample positions of the records: start + dir * dist, one fmaf per axis."""
    ray, step = recs[:, 1].astype(np.int64), recs[:, 2]
    dist = march_dist(stepdist, step)[:, None]
    return fma32(rays_dir[ray], dist, rays_start[ray])


def tri_setup(p, xyz_min, xyz_max, X, Y, Z):
    """-> (ijk0 [E, 3] int64 floor corners, w [E, 8] float32 corner weights, inb [E, 8] bool, vox [E, 8] int64)"""
    p = np.asarray(p, np.float32)
    mn, mx = np.asarray(xyz_min, np.float32), np.asarray(xyz_max, np.float32)
    size1 = np.array([X - 1, Y - 1, Z - 1], np.float32)
    with np.errstate(all='ignore'):
        u = (p - mn) / (mx - mn)
        c = u * _F(2.0) - _F(1.0)
        g = ((c + _F(1.0)) / _F(2.0)) * size1
    assert np.all(np.isfinite(g)), 'non-finite sample position'
    f = np.floor(g)
    w0, w1 = (f + _F(1.0)) - g, g - f                       # [E, 3] each: weight of the floor / the upper corner
    ijk0 = f.astype(np.int64)
    E = p.shape[0]
    w = np.empty((E, 8), np.float32)
    inb = np.empty((E, 8), bool)
    vox = np.empty((E, 8), np.int64)
    dims = (X, Y, Z)
    for q in range(8):
        bit = ((q >> 2) & 1, (q >> 1) & 1, q & 1)
        wx, wy, wz = (np.where(bit[a], w1[:, a], w0[:, a]).astype(np.float32) for a in range(3))
        w[:, q] = (wz * wy) * wx
        ijk = [ijk0[:, a] + bit[a] for a in range(3)]
        inb[:, q] = np.logical_and.reduce([(ijk[a] >= 0) & (ijk[a] < dims[a]) for a in range(3)])
        vox[:, q] = (ijk[0] * Y + ijk[1]) * Z + ijk[2]
    return ijk0, w, inb, vox


def n_bricks(X, Y, Z):
    return tuple((d + BRICK - 1) // BRICK for d in (X, Y, Z))


def _brick_axis(i0, n):
    """dvgo_brick_axis: (b0, b1, count) of the distinct brick coordinates of the in-range voxels {i0, i0 + 1}"""
    i1 = i0 + 1
    in0, in1 = (i0 >= 0) & (i0 < n), (i1 >= 0) & (i1 < n)
    v0, v1 = i0 >> 3, i1 >> 3
    two = in0 & in1 & (v1 != v0)
    b0 = np.where(in0, v0, np.where(in1, v1, 0))
    return b0, np.where(two, v1, 0), np.where(two, 2, np.where(in0 | in1, 1, 0))


def incidences(ijk0, X, Y, Z):
    """The (sample, brick) pairs of the lists: -> (sample index [P], brick id [P]), by sample then brick."""
    BX, BY, BZ = n_bricks(X, Y, Z)
    ax = [_brick_axis(ijk0[:, a], d) for a, d in enumerate((X, Y, Z))]
    smp, brk = [], []
    for cx in range(2):
        for cy in range(2):
            for cz in range(2):
                ok = (ax[0][2] > cx) & (ax[1][2] > cy) & (ax[2][2] > cz)
                b = (ax[0][cx] * BY + ax[1][cy]) * BZ + ax[2][cz]
                idx = np.nonzero(ok)[0]
                smp.append(idx); brk.append(b[idx])
    smp, brk = np.concatenate(smp), np.concatenate(brk)
    order = np.lexsort((brk, smp))
    return smp[order], brk[order]


def voxel_brick(X, Y, Z):
    """brick id of every voxel, [X * Y * Z]"""
    BX, BY, BZ = n_bricks(X, Y, Z)
    i, j, k = np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing='ij')
    return (((i >> 3) * BY + (j >> 3)) * BZ + (k >> 3)).reshape(-1)


# ------------------------------------------------------------------------------------------ the float64 sums
class Sums:
    """ref, mag [n_vox, C + 1] float64 (voxel-major, channel C = density), n, S [n_vox], listed [n_vox] bool."""

    def __init__(self, ref, mag, n, S, listed, shape):
        self.ref, self.mag, self.n, self.S, self.listed, self.shape = ref, mag, n, S, listed, shape

    def __add__(self, other):             # two ranks' lists: the oracle of modes 2 then 3 is the sum of both
        return Sums(self.ref + other.ref, self.mag + other.mag, self.n + other.n, np.maximum(self.S, other.S) + 1,
                    self.listed | other.listed, self.shape)

    def bound(self, atomic=False, k_extra=0):
        k = (self.n + 2 if atomic else self.n + self.S) + k_extra + SLACK
        return gamma(k)[:, None] * self.mag + ((self.n + self.S) * TINY)[:, None] * (self.mag > 0)


def scatter(recs, off, rays_start, rays_dir, stepdist, xyz_min, xyz_max, grad_feat, C, X, Y, Z, slice_len=0,
            by_sample=False):
    """The sums of one launch.  `off`: the list offsets [n_bricks + 1] (entries at and beyond off[-1] are not read).
    `slice_len` > 0: heavy-brick tables are in use.  `by_sample=True`: `recs` is a list of SAMPLES, not of brick lists:
    every in-range corner counts (what grid_sample's backward sums), `off` is ignored."""
    recs = np.ascontiguousarray(recs, np.int32).reshape(-1, 4)
    nvox, CE = X * Y * Z, C + 1
    nb = int(np.prod(n_bricks(X, Y, Z)))
    vb = voxel_brick(X, Y, Z)
    if by_sample:
        E, cnt = recs.shape[0], None
    else:
        off = np.asarray(off, np.int64)
        assert off.shape[0] == nb + 1 and off[0] == 0 and np.all(np.diff(off) >= 0) and off[-1] <= recs.shape[0]
        E, cnt = int(off[-1]), np.diff(off)
    recs = recs[:E]
    ref, mag = np.zeros((nvox, CE)), np.zeros((nvox, CE))
    n = np.zeros(nvox, np.int64)
    if E:
        p = positions(recs, np.asarray(rays_start, np.float32).reshape(-1, 3), np.asarray(rays_dir, np.float32).reshape(-1, 3), stepdist)
        _, w, inb, vox = tri_setup(p, xyz_min, xyz_max, X, Y, Z)
        take = inb.copy()
        if not by_sample:
            brick = np.repeat(np.arange(nb), cnt)
            safe = np.where(inb, vox, 0)
            take &= vb[safe] == brick[:, None]
        e_idx, q_idx = np.nonzero(take)
        v_idx, w_val = vox[e_idx, q_idx], w[e_idx, q_idx].astype(np.float64)
        n = np.bincount(v_idx, minlength=nvox)
        kept = recs[:, 0].astype(np.int64)
        gd = recs[:, 3].copy().view(np.float32).astype(np.float64)
        gf = np.asarray(grad_feat, np.float32).reshape(-1, C) if C else None
        for c in range(CE):
            if c < C:
                g = np.where(kept >= 0, gf[np.maximum(kept, 0), c].astype(np.float64), 0.0)
            else:
                g = gd
            t = w_val * g[e_idx]
            ref[:, c] = np.bincount(v_idx, weights=t, minlength=nvox)
            mag[:, c] = np.bincount(v_idx, weights=np.abs(t), minlength=nvox)
    if by_sample or not slice_len:
        S_b = np.ones(nb, np.int64)
    else:
        S_b = np.maximum(1, -(-cnt // slice_len))
    listed = (cnt > 0)[vb] if cnt is not None else np.ones(nvox, bool)
    return Sums(ref, mag, n, S_b[vb], listed, (X, Y, Z, C))


# ------------------------------------------------------------------------------------------ checks
def _fail(name, bad, *cols):
    idx = np.argwhere(bad)[:5]
    rows = [tuple(int(i) for i in ix) + tuple(float(c[tuple(ix)]) for c in cols) for ix in idx]
    raise AssertionError(f'{name}: {int(bad.sum())} of {bad.size} elements; first (index..., values...): {rows}')


def _voxel_major(gk, gd, shape):
    """k0-shaped [1, C, X, Y, Z] and density-shaped [1, 1, X, Y, Z] arrays -> [n_vox, C + 1]"""
    X, Y, Z, C = shape
    gk = np.moveaxis(np.asarray(gk).reshape(C, X, Y, Z), 0, -1).reshape(-1, C)
    return np.concatenate([gk, np.asarray(gd).reshape(-1, 1)], 1)


def check_dense(O, grad_k0, grad_density, atomic=False, what='brick'):
    """Dense gradients, elementwise: exact zeros where mag == 0, the derived bound elsewhere.  -> worst err / bound"""
    got32 = _voxel_major(grad_k0, grad_density, O.shape)
    got = got32.astype(np.float64)
    if not np.all(np.isfinite(got)):
        _fail(f'{what}: non-finite gradient', ~np.isfinite(got), got)
    zero = O.mag == 0
    if np.any(zero & (got != 0)):
        _fail(f'{what}: non-zero gradient where no term contributes', zero & (got != 0), got)
    err, bound = np.abs(got - O.ref), O.bound(atomic)
    if np.any(err > bound):
        _fail(f'{what}: gradient outside gamma(n + {"2" if atomic else "S"} + {SLACK}) * mag', err > bound, got, O.ref, O.mag,
              np.broadcast_to(O.n[:, None], got.shape))
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.where(bound > 0, err / bound, 0.0)
    return float(r.max()) if r.size else 0.0


class Hyper:
    """The Adam group of dvgo_brick_accumulate as the kernel sees it: float32 values, held as float64."""

    def __init__(self, ss_k0, masked_k0, ss_density, masked_density, beta1, beta2, eps):
        f = lambda x: float(np.float32(x))
        self.ss_k, self.ss_d, self.b1, self.b2, self.eps = f(ss_k0), f(ss_density), f(beta1), f(beta2), f(eps)
        self.masked_k, self.masked_d = bool(masked_k0), bool(masked_density)


def adam_reference(p, g, m, v, ss, b1, b2, eps, masked, perlr=None):
    """The rule itself in float32 numpy, op for op `adam_one` (host test: equals oracle.adam_upd).  In place.
    `perlr` (mode 2, `adam_one<2>`): the step size of an element is fl(ss * perlr)."""
    f = np.float32
    ss, b1, b2, eps = f(ss), f(b1), f(b2), f(eps)
    if perlr is not None:
        ss = ss * np.asarray(perlr, np.float32)
    upd = (g != 0) if masked else np.ones(g.shape, bool)
    m1 = fma32(b1, m, (f(1) - b1) * g)
    v1 = fma32(b2, v, ((f(1) - b2) * g) * g)
    with np.errstate(all='ignore'):
        p1 = p - (ss * m1) / (np.sqrt(v1) + eps)
    p[upd], m[upd], v[upd] = p1[upd], m1[upd], v1[upd]


def check_adam(O, before, after, H, k_extra=0, what='adam', chunk=1 << 19):
    """before / after: (p_k0, m_k0, v_k0, p_density, m_density, v_density) as numpy float32 arrays in the parameters'
    own shapes.  -> dict(undetermined, nonzero, share, updated).  Works through the voxels `chunk` at a time."""
    b6 = [_voxel_major(before[i], before[i + 3], O.shape) for i in range(3)]
    a6 = [_voxel_major(after[i], after[i + 3], O.shape) for i in range(3)]
    tot = dict(undetermined=0, nonzero=0, updated=0)
    for s in range(0, O.n.shape[0], chunk):
        sl = slice(s, s + chunk)
        part = Sums(O.ref[sl], O.mag[sl], O.n[sl], O.S[sl], O.listed[sl], O.shape)
        r = _check_adam_rows(part, [x[sl] for x in b6], [x[sl] for x in a6], H, k_extra, f'{what} (voxels from {s})')
        for k in tot:
            tot[k] += r[k]
    tot['share'] = tot['undetermined'] / max(tot['nonzero'], 1)
    assert tot['share'] <= MAX_UNDETERMINED, f"{what}: {tot['undetermined']} undetermined of {tot['nonzero']} elements with a contribution"
    return tot


def _check_adam_rows(O, before, after, H, k_extra, what):
    (p0, m0, v0), (p1, m1, v1) = before, after
    C = O.shape[3]
    same = [(a.view(np.int32) == b.view(np.int32)) for a, b in ((p0, p1), (m0, m1), (v0, v1))]
    untouched = same[0] & same[1] & same[2]
    p0, m0, v0, p1, m1, v1 = (a.astype(np.float64) for a in (p0, m0, v0, p1, m1, v1))
    for name, a in (('p', p1), ('m', m1), ('v', v1)):
        if not np.all(np.isfinite(a)):
            _fail(f'{what}: non-finite {name}', ~np.isfinite(a), a)
    if np.any(v1 < 0):
        _fail(f'{what}: negative second moment', v1 < 0, v1)
    ss = np.concatenate([np.full(C, H.ss_k), [H.ss_d]])[None, :]
    masked = np.concatenate([np.full(C, H.masked_k), [H.masked_d]])[None, :]
    ref, aref = O.ref, np.abs(O.ref)
    dg = O.bound(False, k_extra)
    u = 1.01 * U
    omb1, omb2 = 1.0 - H.b1, 1.0 - H.b2
    g_m = (m1 - H.b1 * m0) / omb1
    b_m = dg + u * (aref + dg) + (u * np.abs(m1) + 2 * TINY + 2.0 ** -50 * np.abs(m0)) / omb1
    ok_m = np.abs(g_m - ref) <= b_m
    g_v2 = (v1 - H.b2 * v0) / omb2
    b_v = dg * (2 * aref + dg) + 2 * u * (aref + dg) ** 2 + (u * v1 + TINY * (2 + aref + dg) + 2.0 ** -50 * v0) / omb2
    ok_v = np.abs(g_v2 - ref * ref) <= b_v
    step = ss * m1 / (np.sqrt(v1) + H.eps)
    step = np.where(np.isfinite(step), step, 0.0)                         # 0 / (0 + 0): only with eps == 0
    b_p = 1.01 * gamma(4) * np.abs(step) + u * (np.abs(p0) + 1.01 * np.abs(step)) + 5 * TINY
    ok_p = np.abs(p1 - (p0 - step)) <= b_p
    updated = ok_m & ok_v & ok_p
    has = O.mag > 0
    must_stay = (masked & ~has) | (~masked & ~O.listed[:, None])
    must_move = (masked & (aref > dg)) | (~masked & O.listed[:, None])
    und = masked & has & ~(aref > dg)
    for name, s in zip('pmv', same):
        if np.any(must_stay & ~s):
            _fail(f'{what}: {name} changed where no gradient term contributes', must_stay & ~s, p0, p1, m1, v1)
    for name, ok, cols in (('m not (1 - b1) ref + b1 m0', ok_m, (g_m, ref, b_m)), ('v not (1 - b2) ref^2 + b2 v0', ok_v, (g_v2, ref * ref, b_v)),
                           ('p not p0 - ss m1 / (sqrt v1 + eps)', ok_p, (p1, p0 - step, b_p))):
        if np.any(must_move & ~ok):
            _fail(f'{what}: {name}', must_move & ~ok, *cols, m0, m1, v0, v1)
    mixed = und & ~(untouched | updated)
    if np.any(mixed):
        _fail(f'{what}: p, m, v of an undetermined element took different branches', mixed, p0, p1, m0, m1, v0, v1, ref, dg)
    return dict(undetermined=int(und.sum()), nonzero=int(has.sum()), updated=int((must_move | (und & ~untouched)).sum()))


def undetermined_share(O, k_extra=0):
    """On the CPU alone: the share of elements with mag > 0 whose |ref| is within the gradient bound of zero."""
    has = O.mag > 0
    return float((has & ~(np.abs(O.ref) > O.bound(False, k_extra))).sum()) / max(int(has.sum()), 1)


# ------------------------------------------------------------------------------------------ the launch spy
def param_index(fn):
    """{parameter name: position} of an entry point, read from its declaration in include/dvgo_hip.h (the same text
    directvoxgo_amd._lib types the calls from): the spy addresses arguments by NAME, so a reordered or inserted
    parameter moves with its name instead of being mis-read."""
    import os
    import re
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(os.path.dirname(here), 'include', 'dvgo_hip.h')) as f:
        text = re.sub(r'/\*.*?\*/', ' ', f.read(), flags=re.S)
    m = re.search(r'\b%s\s*\(([^)]*)\)' % re.escape(fn), text)
    assert m is not None, f'include/dvgo_hip.h does not declare {fn}'
    names = [re.search(r'(\w+)\s*$', p).group(1) for p in m.group(1).split(',')]
    assert len(set(names)) == len(names)
    return {n: i for i, n in enumerate(names)}


_ACC = param_index('dvgo_brick_accumulate')
A_OFF, A_EXTRA_OFF, A_SLICE, A_RECS = (_ACC[k] for k in ('brick_off', 'extra_off', 'slice_len', 'recs'))
A_START, A_DIRS, A_STEPDIST, A_MIN, A_MAX = (_ACC[k] for k in ('rays_start', 'rays_dir', 'stepdist', 'xyz_min', 'xyz_max'))
A_GFEAT, A_C, A_X, A_GK, A_GD = (_ACC[k] for k in ('grad_feat', 'C', 'X', 'grad_k0', 'grad_density'))
A_ADAM, A_SS_DEV, A_TILES, A_MODE, N_ARGS = _ACC['p_k0'], _ACC['step_sizes_dev'], _ACC['tiles'], _ACC['tiles_mode'], len(_ACC)
# the Adam group p_k0 .. step_sizes_dev is read as one run of 14 (fused._NO_ADAM, MaskedAdam.grid_step_args)
_ADAM_RUN = ('p_k0', 'm_k0', 'v_k0', 'step_size_k0', 'masked_k0', 'p_density', 'm_density', 'v_density', 'step_size_density',
             'masked_density', 'beta1', 'beta2', 'eps', 'step_sizes_dev')
assert [_ACC[k] - A_ADAM for k in _ADAM_RUN] == list(range(14)) and (_ACC['Y'], _ACC['Z']) == (A_X + 1, A_X + 2)


def _np(t):
    return t.detach().cpu().numpy()


def _f3(x):
    return np.array([float(v) for v in x], np.float32)


class Launch:
    """One observed dvgo_brick_accumulate: `sums` (the oracle of its inputs), `kind` ('dense' | 'adam' | 'tiles'), and what
    the checks returned (`worst` err / bound of the dense gradients, `adam` the dict of check_adam)."""
    sums = kind = worst = adam = hyper = inputs = None


class LaunchSpy(contextlib.AbstractContextManager):
    """with LaunchSpy() as spy: ...  Every dvgo_brick_accumulate issued inside (modes 0 and 1) is held to the oracle when it
    returns; `spy.launches` keeps one `Launch` each, `spy.calls` the name of every entry point called.  `check=False` only records the sums (the caller compares)."""

    def __init__(self, check=True):
        self.check, self.launches, self.calls = check, [], []

    def __enter__(self):
        from directvoxgo_amd import _lib as L
        self._L, self._orig = L, L.call
        L.call = self._call
        return self

    def __exit__(self, *exc):
        self._L.call = self._orig
        return False

    def _call(self, name, *args):
        self.calls.append(name)
        if name != 'dvgo_brick_accumulate' or args[A_MODE] != 0:
            return self._orig(name, *args)
        import torch
        assert len(args) == N_ARGS
        adam = args[A_ADAM] is not None
        torch.cuda.synchronize()
        X, Y, Z = args[A_X:A_X + 3]
        C = args[A_C]
        off = _np(args[A_OFF])
        recs = _np(args[A_RECS][:int(off[-1])])
        ins = dict(recs=recs, off=off, rays_start=_np(args[A_START]), rays_dir=_np(args[A_DIRS]), stepdist=args[A_STEPDIST],
                   xyz_min=_f3(args[A_MIN]), xyz_max=_f3(args[A_MAX]), grad_feat=_np(args[A_GFEAT]), C=C, X=X, Y=Y, Z=Z,
                   slice_len=args[A_SLICE] if args[A_EXTRA_OFF] is not None else 0)
        grids = [args[A_ADAM + i] for i in (0, 1, 2, 5, 6, 7)] if adam else None
        before = [_np(t).copy() for t in grids] if adam else None
        self._orig(name, *args)
        torch.cuda.synchronize()
        rec = Launch()
        rec.inputs = ins
        rec.sums = scatter(**ins)
        rec.kind = 'adam' if adam else 'dense'
        rec.n_rec_rows = int(args[A_RECS].shape[0])
        rec.ss_from_device = bool(adam and args[A_SS_DEV] is not None)
        if adam:
            a = args[A_ADAM:A_ADAM + 14]
            ss_k, ss_d = (a[3], a[8]) if a[13] is None else (float(x) for x in _np(a[13])[:2])
            rec.hyper = Hyper(ss_k, a[4], ss_d, a[9], a[10], a[11], a[12])
            rec.before, rec.after = before, [_np(t).copy() for t in grids]
            if self.check:
                rec.adam = check_adam(rec.sums, rec.before, rec.after, rec.hyper)
        else:
            rec.grads = (_np(args[A_GK]).copy(), _np(args[A_GD]).copy())
            if self.check:
                rec.worst = check_dense(rec.sums, *rec.grads)
        self.launches.append(rec)


# ------------------------------------------------------------------------------------------ synthetic lists
def synthetic(dims, C, spec, seed=0, family='random', drop=0.1):
    """Hand-made brick lists at the library boundary: one "ray" per record with rays_dir = 0, so a record's position is its
    rays_start.  spec: [((bx, by, bz), count, kind)], kind
        'interior'  floor corner and upper corner inside the brick (and the lattice): all eight corners are the brick's
        'one_voxel' as 'interior', every record at the same position (256 records -> 2048 references, 256 per voxel)
        'corner'    floor corner one below the brick's low corner: only corner 7 is the brick's (needs bx, by, bz > 0)
        'max'       on xyz_max along every axis where the brick is the last one (weights 1 and 0, upper corners out of range)
    family: 'random' g ~ N(0, 1); 'correlated' g = |N(0, 1)| (one sign: nothing cancels); 'shifted' g ~ N(0.5, 1).
    `drop`: share of records with kept index -1 (no feature gradient).  In every brick a quarter of the feature channels
    is exactly zero (see below).  -> dict of `scatter` inputs plus 'counts'."""
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    B = n_bricks(X, Y, Z)
    nb = int(np.prod(B))
    mn, mx = np.array([-1.0, -0.75, -1.25], np.float32), np.array([1.0, 1.25, 0.75], np.float32)
    counts = np.zeros(nb, np.int64)
    chunks = []
    for (bx, by, bz), count, kind in spec:
        b = (bx * B[1] + by) * B[2] + bz
        assert 0 <= bx < B[0] and 0 <= by < B[1] and 0 <= bz < B[2] and counts[b] == 0 and count > 0
        g = np.empty((count, 3))
        for a, (ba, size, nba) in enumerate(zip((bx, by, bz), dims, B)):
            lo = 8 * ba
            hi = min(lo + 6, size - 2)                      # highest floor corner with the upper corner in brick and lattice
            if kind == 'corner':
                assert ba > 0
                g[:, a] = lo - 1 + rng.uniform(0.1, 0.9, count)
            elif kind == 'max' and ba == nba - 1:
                g[:, a] = size - 1
            elif hi < lo:
                raise AssertionError('brick too thin for an interior sample')
            elif kind == 'one_voxel':
                g[:, a] = lo + (hi - lo) // 2 + (0.3, 0.55, 0.7)[a]
            else:
                g[:, a] = rng.integers(lo, hi + 1, count) + rng.uniform(0.1, 0.9, count)
        counts[b] = count
        chunks.append((b, g, kind))
    chunks.sort(key=lambda c: c[0])
    g = np.concatenate([c[1] for c in chunks])
    size1 = np.array([X - 1, Y - 1, Z - 1], np.float64)
    pos = (mn.astype(np.float64) + g / size1 * (mx.astype(np.float64) - mn)).astype(np.float32)
    on_max = np.concatenate([np.broadcast_to(np.array([c[2] == 'max' and ba == nba - 1 for ba, nba in
                                                       zip(np.unravel_index(c[0], B), B)]), c[1].shape) for c in chunks])
    pos = np.where(on_max, mx[None, :], pos)
    E = pos.shape[0]
    kept = np.arange(E, dtype=np.int64)
    dropped = rng.uniform(size=E) < drop
    kept = np.where(dropped, -1, np.cumsum(~dropped) - 1)
    M = int((~dropped).sum())
    draw = {'random': lambda s: rng.standard_normal(s), 'correlated': lambda s: np.abs(rng.standard_normal(s)),
            'shifted': lambda s: rng.standard_normal(s) + 0.5}[family]
    gf = draw((max(M, 1), C)).astype(np.float32)
    gd = draw(E).astype(np.float32)
    # exact zeros: in the j-th listed brick the feature channels c = j mod 4 (mod 4) are zero in every record, so its
    # voxels have gradients that are exactly 0 in one lane of each float4 and non-zero in the others: the masked rule
    # is per element, wherever in the float4 the zero sits
    first = 0
    for j, (b, gb, _) in enumerate(chunks):
        rows = kept[first:first + gb.shape[0]]
        gf[rows[rows >= 0], j % 4::4] = 0
        first += gb.shape[0]
    recs = np.empty((E, 4), np.int32)
    recs[:, 0], recs[:, 1], recs[:, 2], recs[:, 3] = kept, np.arange(E), np.arange(E) % 7, gd.view(np.int32)
    off = np.concatenate([[0], np.cumsum(counts)])
    ins = dict(recs=recs, off=off, rays_start=pos, rays_dir=np.zeros_like(pos), stepdist=0.5, xyz_min=mn, xyz_max=mx,
               grad_feat=gf, C=C, X=X, Y=Y, Z=Z)
    # the table is checked here, before anything is launched from it: every record's intended floor corner is the one
    # the float32 setup finds, every index is inside its buffer, every listed record has a corner in its brick
    ijk0, w, inb, vox = tri_setup(pos, mn, mx, X, Y, Z)
    assert np.array_equal(ijk0, np.floor(g).astype(np.int64)), 'float32 setup moved a floor corner'
    assert recs[:, 0].max(initial=-1) < gf.shape[0] and recs[:, 0].min() >= -1 and recs[:, 1].max() < pos.shape[0]
    brick = np.repeat(np.arange(nb), counts)
    mine = inb & (voxel_brick(X, Y, Z)[np.where(inb, vox, 0)] == brick[:, None])
    assert np.all(mine.any(1)), 'a record has no corner in the brick that lists it'
    return dict(ins, counts=counts)


def slice_edge_spec(dims, slice_len):
    """The list lengths at the 256-entry chunk edge and the slice edge, one brick each, spread over the lattice (bricks of
    the last, partial layer of every axis included), with the exactly-full `refs` cases, a corner-only brick and records
    on xyz_max."""
    B = n_bricks(*dims)
    lengths = [1, 255, 256, 257, 511, 512, slice_len - 1, slice_len, slice_len + 1, 2 * slice_len, 3 * slice_len + 7]
    fat = lambda b: all(min(8 * ba + 6, size - 2) >= 8 * ba for ba, size in zip(b, dims))
    last = (B[0] - 1, B[1] - 1, B[2] - 1)
    bricks = [(x, y, z) for x in range(B[0]) for y in range(B[1]) for z in range(B[2]) if (x, y, z) != last]
    inner = [b for b in bricks if min(b) > 0]
    spec = [(inner[0], 256, 'corner'), (last, 300, 'max')]
    free = [b for b in bricks if fat(b) and b != inner[0]]
    free.sort(key=lambda b: -sum(ba == nba - 1 for ba, nba in zip(b, B)))      # partial layers first
    spec.append((free.pop(len(free) // 2), 512, 'one_voxel'))
    for n in lengths:
        spec.append((free.pop(0), n, 'interior'))
    return spec


# two slice lengths: 256 is one chunk per slice (the smallest the library accepts); with 1024 a slice is several chunks, so
# the slices k >= 1 run the multi-chunk loop with its prefetch (lists of 1023 / 1024 / 1025 / 2048 / 3079 entries, the
# last one with a ragged chunk inside its last slice), and the chunk edge and the slice edge are different lengths
SYN_DIMS, SYN_SLICE, SYN_SLICES = (20, 23, 18), 256, (256, 1024)
SYN_FAMILIES = ('random', 'correlated', 'shifted')


def rank_specs(dims=SYN_DIMS, slice_len=SYN_SLICE):
    """Two lists standing in for two ranks: A = the edge lengths; B shares A's heaviest brick (both sliced) and two more,
    and has one brick A never touches; most of A's bricks B never touches."""
    A = slice_edge_spec(dims, slice_len)
    by_len = sorted((s for s in A if s[2] == 'interior'), key=lambda s: s[1])
    used = {s[0] for s in A}
    B3 = n_bricks(*dims)
    fresh = next(b for b in ((x, y, z) for x in range(B3[0]) for y in range(B3[1]) for z in range(B3[2]))
                 if b not in used and all(min(8 * ba + 6, size - 2) >= 8 * ba for ba, size in zip(b, dims)))
    B = [(by_len[-1][0], 2 * slice_len + 3, 'interior'), (by_len[0][0], 300, 'interior'), (by_len[3][0], 40, 'interior'),
         (fresh, 2 * slice_len, 'interior')]
    return A, B


def synthetic_case(family, C, rank='A', slice_len=SYN_SLICE):
    """The inputs every synthetic GPU test launches from, by family and channel count (the host test measures the
    undetermined share of exactly these).  The all-on-one-voxel brick is part of every case."""
    A, B = rank_specs(SYN_DIMS, slice_len)
    seed = 1000 * SYN_FAMILIES.index(family) + 10 * C + (rank == 'B') + slice_len
    ins = synthetic(SYN_DIMS, C, A if rank == 'A' else B, seed=seed, family=family)
    counts = ins.pop('counts')
    return ins, counts
