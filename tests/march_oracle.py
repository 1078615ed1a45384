"""Float64 statement of the fused march per sample (test infrastructure, CPU only): csrc/march.hip's transmittance chain
-- march_density, march_gather, march_composite, march_composite_bwd, march_density_bwd -- from what crosses the library
boundary (include/dvgo_hip.h; arguments are found by the header's names, `brick_oracle.param_index`).

u = 2^-24, gamma(k) = k u / (1 - k u) (Higham, Lemma 3.1), TINY = 2^-149 per operation whose result may be subnormal, SLACK
= 1 covers this file's own float64 arithmetic (n 2^-53 mag < u mag) and second-order terms.  No constant here was fitted
to GPU output.

EXACT (bit for bit), on the `rec2` records {step | flag << 31, exp_d, alpha, T} of every ray  -- `check_records`
  T_0 == 1 and T_{j+1} == float32(float64(T_j) * (1.0 - float64(alpha_j) + 1e-10)): the kernel's operation sequence
      (widen, one double multiply by the double factor, narrow), which numpy reproduces exactly; independent of the C oracle.
  stop   T_after := the same expression of the record itself.  No record but a ray's last has T_after < 1e-3 (compared as
      `(double)T_after < 1e-3`), and alphainv_last == T_after of the last record (1.0 for a ray without records).  That a ray
      whose last record has T_after >= 1e-3 has no later candidate step is a statement about the density grid, which the
      records do not hold: it is made where a forward oracle exists (tests/march_cases.py compares n2 and the stop step with
      the CPU oracle's; tests/test_gpu_fullsize_oracle.py compares the ids).
  NaN    a NaN alpha (possible only with thres == 0: `NaN > thres` is false) makes T NaN; `NaN < 1e-3` is false, so the
      reference does not stop.  The kernel compares the bit pattern unsigned against 0x3a83126f: a NaN's exponent is all
      ones, its pattern is above, no stop either: both agree, and every index stays the step count's.  The recurrence above
      is checked on bit patterns of the value float32(NaN-product), which numpy also yields as NaN; NaN payloads are not
      compared (`_same` treats two NaNs as equal).
  flag   bit 31 set iff float32(T * alpha) > thres (always when thres == 0); n3 == number of flags; n2 == number of
      records; steps strictly increase and are < n_steps; with thres > 0 every record has alpha > thres.
  gather -- `check_gather`: off3 == exclusive scan of n3; weights == float32(T * alpha), alpha, ray_id, step_id of the
      flagged records in ray-major order at off3[r] + rank.

BOUNDED, per element, float64 reference from the kernel's own float32 inputs
  composite -- `check_composite`: per ray (n samples) and channel ref = sum w c + last bg, mag = sum |w c| + |last bg|.
      Lane l forms its partial sum by one fmaf per sample l, l + 64, ... (ceil(n / 64) roundings on a term's path; the
      padding lanes add w = 0 exactly), the butterfly adds 6 times, `last * bg` is one rounding and joins by one addition:
          |got - ref| <= gamma(ceil(n / 64) + 6 + 1 + SLACK) mag + (n + 2) TINY.         Depth: c = step_id, no last term.
  composite_bwd -- `check_composite_bwd`:
      grad_weights = fmaf(g2, c2, fmaf(g1, c1, fl(g0 c0))): 3 roundings, gamma(3 + SLACK) (|g0 c0| + |g1 c1| + |g2 c2|) + 3 TINY
      grad_rgb     = fl(g w), or fmaf(g, w, before) under `accumulate`: one rounding, (1 + SLACK) u |ref| + TINY
      grad_last    = fl(fl(fl(g0 + g1) + g2) bg) [+ before]: two additions, one product, one optional addition:
                     gamma(4 + SLACK) ((|g0| + |g1| + |g2|) |bg| + |before|) + 2 TINY
  density_bwd -- `density_bwd_reference` / `check_density_bwd`: record i (0-based) of a ray with n records, w_j =
      float32(T_j alpha_j), g_w_j the upstream gradient of a flagged record and 0 otherwise:
          A_i = g_last last + sum_{j > i} g_w_j w_j        magA_i = the same with absolute values
          g_alpha_ref = g_w_i T_i - A_i / (float64(float32(1 - alpha_i)) + 1e-10)
      What a float32 evaluation rounds: every product g_w_j w_j and g_last last once; the additions that join them; gt =
      fl(g_w_i T_i) once; the subtraction and the division are double; the result is rounded once.  With k_i roundings on the
      longest path of a term of A_i:
          |got - ref| <= (u |g_w_i T_i| + gamma(k_i) magA_i / den_i) (1 + 2u) + u |ref| + ((n - i) + 2) TINY / den_i + TINY
      k_i depends on the order of summation, a parameter of the bound:
        'tree'   march_density_bwd_kernel: chunks of 64 records from the far end, q_i = floor((n - 1 - i) / 64) chunks lie
                 beyond record i's own.  A term of a farther chunk: 1 (product) + 6 (`wave_suffix_excl`: log2 64 additions
                 to reach lane 0's total) + at most q_i (`acc += total`, once per chunk from its own to the one before
                 i's) + 1 (`acc + suffix`); a term of i's own chunk: 1 + 6 + 1; g_last last: 1 + q_i + 1.
                 k_i = 8 + q_i + SLACK.
        'serial' the reference's walk `back_cum += g_w w` from the far end (oracle/dvgo_oracle.c, fma or plain): 1 (product;
                 none under fma) + (n - 1 - i) additions.  k_i = (n - i) + SLACK.
      The bound follows the conditioning: it is large only where den_i is small (alpha -> 1) or A_i cancels g_w_i T_i, and
      there the reference's own float32 evaluation is as uncertain.
      g_d = float32(min(e, 1e10) * p * interval * g_alpha), p = dvgo_pow_neg(float32(1 + e), float32(-interval - 1)) =
      exp2(y log2 x) on v_log_f32 / v_exp_f32.  Their accuracy is not documented in the guides this project has; the
      allowance is the project's own stated and tested figure for this function, POW_RTOL = 1e-5 relative (csrc/common.h,
      comment of dvgo_pow_neg; tests/test_gpu_ops.py test_raw2alpha) -- a tested figure, not a derivation.  v_exp_f32 may flush a
      result below 2^-126 to zero: POW_FLUSH = 2^-126 absolute on p.  With F = min(e, 1e10) interval:
          |got - ref| <= (F (p (1 + POW_RTOL) + POW_FLUSH) dga + F (p POW_RTOL + POW_FLUSH) |g_alpha_ref|) (1 + u) + u |ref| + TINY
      where dga is the g_alpha bound.  p is evaluated in float64 from x = float32(1 + e), as the reference forms it.
  zero rule: a ray whose g_w are all 0 and whose g_last is 0 (or NULL) has g_d == 0.0 in every record.
  Where g_d is read: on the brick path from EVERY list entry (`brick_recs[...].w`; the up to 8 entries of one sample must be
  bit-identical, every record must be listed, the kept index must be off3[r] + rank or -1); on the atomic path from
  `grad_kept` for flagged records when it is given, and the rest through `grad_density`: per voxel, n contributions,
          |got - ref| <= sum |w_tri| dgd + gamma(n + 2 + SLACK) (sum |w_tri| (|g_d_ref| + dgd)) + n TINY
  (`brick_oracle`'s `atomic` count: product, table additions, memory additions), exact 0 where nothing contributes.
Every record of every ray is compared; nothing is classed undetermined and nothing is skipped.

`MarchSpy` extends `brick_oracle.LaunchSpy` (one mechanism: the same wrap of `directvoxgo_amd._lib.call`): the five march
entry points are checked on their actual arguments when they return; `report` keeps (records checked, worst err / bound).
Launches issued while a graph is being captured cannot be observed (no synchronisation there) and pass through unchecked.
"""
import numpy as np

import brick_oracle as B
from brick_oracle import SLACK, TINY, U, gamma

POW_RTOL = 1e-5
POW_FLUSH = 2.0 ** -126
_F = np.float32


# ------------------------------------------------------------------------------------------ records
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same(a, b):
    """bit-identical float32 arrays; two NaNs count as the same value"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


def _fail(what, bad, R, *cols):
    idx = np.nonzero(bad)[0][:5]
    rows = []
    for i in idx:
        n = int(R.n[R.ray[i]])
        rows.append(dict(ray=int(R.ray[i]), record=int(R.idx[i]), of=n, step=int(R.step[i]), lane=int(R.step[i]) % 64,
                         bwd_chunk=(n - 1 - int(R.idx[i])) // 64, values=[float(c[i]) for c in cols]))
    raise AssertionError(f'{what}: {int(bad.sum())} of {bad.size} records; first: {rows}')


class Records:
    """The rec2 records of a launch in ray-major order.  rec2: [rows, 4] float32 as the device holds it, n2 [N], base [N]
    the row of each ray's first record.  step, flag, exp_d, alpha, T [E]; ray, idx (position in its ray) [E]; n = n2."""

    def __init__(self, rec2, n2, base):
        rec2 = np.ascontiguousarray(rec2, np.float32).reshape(-1, 4)
        self.n = n = np.asarray(n2, np.int64)
        base = np.asarray(base, np.int64)
        assert np.all(n >= 0) and (n.size == 0 or np.all(base + n <= rec2.shape[0])), 'n2 runs past the record buffer'
        self.first = np.concatenate([[0], np.cumsum(n)])
        self.ray = np.repeat(np.arange(n.shape[0]), n)
        self.idx = np.arange(self.ray.shape[0]) - self.first[self.ray]
        raw = rec2[base[self.ray] + self.idx]
        s = np.ascontiguousarray(raw[:, 0]).view(np.int32)
        self.flag, self.step = s < 0, (s & 0x7fffffff).astype(np.int64)
        self.exp_d, self.alpha, self.T = (np.ascontiguousarray(raw[:, c]) for c in (1, 2, 3))
        self.is_last = self.idx == n[self.ray] - 1
        with np.errstate(all='ignore'):
            self.T_after = (self.T.astype(np.float64) * (1.0 - self.alpha.astype(np.float64) + 1e-10)).astype(np.float32)
            self.w = self.T * self.alpha

    @property
    def rank(self):
        """position of a flagged record among its ray's flagged records"""
        c = np.cumsum(self.flag) - self.flag
        return c - np.append(c, 0)[self.first[:-1]][self.ray]          # (a ray without records may start at E)


def rec_base(n_steps, cum, rec_stride):
    n_steps = np.asarray(n_steps, np.int64)
    return (np.asarray(cum, np.int64) - n_steps) if cum is not None else np.arange(n_steps.shape[0], dtype=np.int64) * int(rec_stride)


def check_records(R, n_steps, thres, n3, last):
    """The exact checks of march_density.  -> number of records"""
    thres = _F(thres)
    n_steps, n3, last = np.asarray(n_steps, np.int64), np.asarray(n3, np.int64), np.asarray(last, np.float32)
    E = R.ray.shape[0]
    first = R.idx == 0
    if np.any(first & ~_same(R.T, np.ones(E, np.float32))):
        _fail('T of a ray\'s first record is not 1', first & ~_same(R.T, np.ones(E, np.float32)), R, R.T)
    nxt = ~R.is_last
    bad = np.zeros(E, bool)
    bad[:-1] = nxt[:-1] & ~_same(R.T[1:], R.T_after[:-1])
    if bad.any():
        _fail('T_{j+1} != float32(double(T_j) * (1 - alpha_j + 1e-10))', bad, R, R.T, R.alpha, R.T_after)
    stopped = R.T_after.astype(np.float64) < 1e-3
    if np.any(nxt & stopped):
        _fail('a record before the last has T_after < 1e-3 (the ray went on after its stop)', nxt & stopped, R, R.T, R.alpha, R.T_after)
    want_last = np.ones(R.n.shape[0], np.float32)
    want_last[R.ray[R.is_last]] = R.T_after[R.is_last]
    assert np.all(_same(last, want_last)), ('alphainv_last is not T_after of the last record', np.nonzero(~_same(last, want_last))[0][:5])
    want_flag = (R.w > thres) if thres > 0 else np.ones(E, bool)
    if np.any(R.flag != want_flag):
        _fail('bit 31 is not float32(T * alpha) > thres', R.flag != want_flag, R, R.T, R.alpha, R.w)
    assert np.array_equal(np.bincount(R.ray, R.flag, R.n.shape[0]).astype(np.int64), n3), 'n3 is not the number of flagged records'
    bad = (R.step >= n_steps[R.ray])
    bad[1:] |= ~first[1:] & (R.step[1:] <= R.step[:-1])
    if bad.any():
        _fail('steps do not strictly increase below n_steps', bad, R, R.step)
    if thres > 0 and np.any(~(R.alpha > thres)):
        _fail('a record has alpha <= thres', ~(R.alpha > thres), R, R.alpha)
    return E


def check_gather(R, n3, off3, ray_id, step_id, weights, alpha):
    """march_gather's ids and weights: the flagged records in ray-major order.  -> number of samples"""
    n3 = np.asarray(n3, np.int64)
    want_off = np.concatenate([[0], np.cumsum(n3)])
    assert np.array_equal(np.asarray(off3, np.int64)[:want_off.shape[0]], want_off), 'off3 is not the exclusive scan of n3'
    M = int(want_off[-1])
    k = R.flag
    assert int(k.sum()) == M
    pos = want_off[R.ray[k]] + R.rank[k]
    assert np.array_equal(pos, np.arange(M)), 'off3[r] + rank is not the ray-major order'
    for name, got, want in (('ray_id', ray_id, R.ray[k]), ('step_id', step_id, R.step[k])):
        assert np.array_equal(np.asarray(got)[:M], want), f'{name} of the gathered samples'
    for name, got, want in (('weights', weights, R.w[k]), ('alpha', alpha, R.alpha[k])):
        ok = _same(np.asarray(got)[:M], want)
        assert np.all(ok), (f'{name} != the record\'s', np.nonzero(~ok)[0][:5])
    return M


# ------------------------------------------------------------------------------------------ per-ray sums
def _ratio(err, bound):
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def _hold(what, got, ref, bound):
    got = np.asarray(got, np.float64)
    bad = ~(np.abs(got - ref) <= bound)
    if bad.any():
        ix = np.argwhere(bad)[:5]
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.size} outside the bound; first (index, got, ref, bound): '
                             f'{[(tuple(int(v) for v in i), float(got[tuple(i)]), float(ref[tuple(i)]), float(bound[tuple(i)])) for i in ix]}')
    return _ratio(np.abs(got - ref), bound)


def check_composite(weights, rgb, step_id, off3, last, bg, rgb_marched, depth=None):
    """-> worst err / bound over rgb_marched (and depth)"""
    off3 = np.asarray(off3, np.int64)
    N = off3.shape[0] - 1
    n = np.diff(off3)
    M = int(off3[-1])
    ray = np.repeat(np.arange(N), n)
    w = np.asarray(weights, np.float64)[:M] if M else np.zeros(0)
    c = np.asarray(rgb, np.float64).reshape(-1, 3)[:M] if M else np.zeros((0, 3))
    lb = np.asarray(last, np.float64) * float(_F(bg))
    k = -(-n // 64) + 6 + 1 + SLACK
    ref, mag = np.empty((N, 3)), np.empty((N, 3))
    for ch in range(3):
        t = w * c[:, ch]
        ref[:, ch] = np.bincount(ray, t, N) + lb
        mag[:, ch] = np.bincount(ray, np.abs(t), N) + np.abs(lb)
    bound = gamma(k)[:, None] * mag + ((n + 2) * TINY)[:, None]
    worst = _hold('march_composite rgb_marched', np.asarray(rgb_marched).reshape(N, 3), ref, bound)
    if depth is not None:
        t = w * np.asarray(step_id, np.float64)[:M]
        worst = max(worst, _hold('march_composite depth', depth, np.bincount(ray, t, N), gamma(k) * np.bincount(ray, np.abs(t), N) + (n + 2) * TINY))
    return worst


def check_composite_bwd(gout, weights, rgb, ray_id, M, bg, grad_weights, grad_rgb, grad_last, before_rgb=None, before_last=None):
    """`before_*`: what grad_rgb / grad_last held before an accumulating launch (None: a plain one).  -> worst err / bound"""
    g = np.asarray(gout, np.float64).reshape(-1, 3)
    worst = 0.0
    if M:
        gr = g[np.asarray(ray_id, np.int64)[:M]]
        c, w = np.asarray(rgb, np.float64).reshape(-1, 3)[:M], np.asarray(weights, np.float64)[:M]
        if grad_weights is not None:
            t = gr * c
            worst = max(worst, _hold('composite_bwd grad_weights', np.asarray(grad_weights)[:M], t.sum(1), gamma(3 + SLACK) * np.abs(t).sum(1) + 3 * TINY))
        if grad_rgb is not None:
            ref = gr * w[:, None] + (0.0 if before_rgb is None else np.asarray(before_rgb, np.float64).reshape(-1, 3)[:M])
            worst = max(worst, _hold('composite_bwd grad_rgb', np.asarray(grad_rgb).reshape(-1, 3)[:M], ref, (1 + SLACK) * U * np.abs(ref) + TINY))
    if grad_last is not None:
        b = float(_F(bg))
        prev = 0.0 if before_last is None else np.asarray(before_last, np.float64)
        ref, mag = g.sum(1) * b + prev, np.abs(g).sum(1) * abs(b) + np.abs(prev)
        worst = max(worst, _hold('composite_bwd grad_last', grad_last, ref, gamma(4 + SLACK) * mag + 2 * TINY))
    return worst


# ------------------------------------------------------------------------------------------ the density backward
def _suffix_excl(R, t, block=1 << 22):
    """per record: sum of t over the later records of its ray, in float64 within the ray (never across rays)"""
    out = np.zeros(t.shape[0])
    N = R.n.shape[0]
    if not t.shape[0]:
        return out
    nmax = int(R.n.max())
    per = max(1, block // max(nmax, 1))
    for r0 in range(0, N, per):
        r1 = min(N, r0 + per)
        a, b = int(R.first[r0]), int(R.first[r1])
        if a == b:
            continue
        P = np.zeros((r1 - r0, nmax))
        P[R.ray[a:b] - r0, R.idx[a:b]] = t[a:b]
        S = np.cumsum(P[:, ::-1], axis=1)[:, ::-1] - P
        out[a:b] = S[R.ray[a:b] - r0, R.idx[a:b]]
    return out


def gw_per_record(R, off3, grad_weights):
    """upstream gradient of every record: grad_weights[off3[r] + rank] where flagged, 0 elsewhere (float32)"""
    gw = np.zeros(R.ray.shape[0], np.float32)
    k = R.flag
    if k.any():
        gw[k] = np.asarray(grad_weights, np.float32)[np.asarray(off3, np.int64)[R.ray[k]] + R.rank[k]]
    return gw


class DensityBwdRef:
    """ga, dga (g_alpha reference and bound), gd, dgd (g_d reference and bound), zero (records under the zero rule)"""


def density_bwd_reference(R, last, gw, g_last, interval, order='tree'):
    """gw [E] float32 per record (`gw_per_record`), g_last [N] float32 or None.  `order`: 'tree' | 'serial' (module text)."""
    assert order in ('tree', 'serial')
    N = R.n.shape[0]
    last64 = np.asarray(last, np.float64)
    gl = np.zeros(N) if g_last is None else np.asarray(g_last, np.float64)
    n, i = R.n[R.ray], R.idx
    with np.errstate(all='ignore'):
        t = gw.astype(np.float64) * R.w.astype(np.float64)
        head = (gl * last64)[R.ray]
        A = head + _suffix_excl(R, t)
        magA = np.abs(head) + _suffix_excl(R, np.abs(t))
        den = (_F(1.0) - R.alpha).astype(np.float64) + 1e-10
        gt = gw.astype(np.float64) * R.T.astype(np.float64)
        O = DensityBwdRef()
        O.ga = gt - A / den
        k = (8 + (n - 1 - i) // 64 + SLACK) if order == 'tree' else ((n - i) + SLACK)
        O.dga = (U * np.abs(gt) + gamma(k) * magA / den) * (1 + 2 * U) + U * np.abs(O.ga) + ((n - i) + 2) * TINY / den + TINY
        e = R.exp_d.astype(np.float64)
        x = (_F(1.0) + R.exp_d).astype(np.float64)
        y = float(-_F(interval) - _F(1.0))
        p = np.power(x, y)
        F = np.minimum(e, 1e10) * float(_F(interval))
        O.gd = np.where(p == 0, 0.0, F * p) * O.ga
        O.dgd = (F * (p * (1 + POW_RTOL) + POW_FLUSH) * O.dga + F * (p * POW_RTOL + POW_FLUSH) * np.abs(O.ga)) * (1 + U) + U * np.abs(O.gd) + TINY
    quiet = (np.bincount(R.ray, gw != 0, N) == 0) & (gl == 0)
    O.zero = quiet[R.ray]
    return O


def check_density_bwd(R, O, g_d, what='march_density_bwd'):
    """g_d [E] float32 per record against the reference.  -> worst err / bound"""
    got = np.asarray(g_d, np.float64)
    if np.any(O.zero & (got != 0)):
        _fail(f'{what}: zero rule (no upstream gradient on the ray, g_d != 0)', O.zero & (got != 0), R, got)
    fin = np.isfinite(O.gd) & np.isfinite(O.dgd)
    bad = fin & ~(np.abs(got - O.gd) <= O.dgd)
    bad |= ~fin & np.isfinite(O.gd) & ~np.isfinite(got)
    if bad.any():
        _fail(f'{what}: g_d outside its bound (got, ref, bound, g_alpha ref, alpha, T, exp_d)', bad, R, got, O.gd, O.dgd, O.ga, R.alpha, R.T, R.exp_d)
    return _ratio(np.abs(got - O.gd)[fin], O.dgd[fin])


def check_density_scatter(R, O, sel, rays_start, rays_dir, stepdist, xyz_min, xyz_max, dims, got, what='grad_density'):
    """The records `sel` scattered into a dense grid by float atomics: per voxel against the float64 scatter of the
    reference g_d, `brick_oracle`'s atomic count widened by the per-sample bound.  -> worst err / bound"""
    X, Y, Z = dims
    nvox = X * Y * Z
    got = np.asarray(got, np.float64).reshape(nvox)
    ix = np.nonzero(sel & ~O.zero)[0]
    ref, mag, dsum, n = np.zeros(nvox), np.zeros(nvox), np.zeros(nvox), np.zeros(nvox, np.int64)
    if ix.size:
        recs = np.stack([np.zeros_like(ix), R.ray[ix], R.step[ix], np.zeros_like(ix)], 1).astype(np.int32)
        p = B.positions(recs, np.asarray(rays_start, np.float32).reshape(-1, 3), np.asarray(rays_dir, np.float32).reshape(-1, 3), stepdist)
        _, w, inb, vox = B.tri_setup(p, xyz_min, xyz_max, X, Y, Z)
        e, q = np.nonzero(inb)
        v, wv = vox[e, q], np.abs(w[e, q].astype(np.float64))
        sg = np.sign(w[e, q].astype(np.float64))
        fin = np.isfinite(O.dgd[ix])
        assert fin.all(), f'{what}: a scattered record has no finite bound'
        ref = np.bincount(v, sg * wv * O.gd[ix][e], nvox)
        mag = np.bincount(v, wv * (np.abs(O.gd[ix]) + O.dgd[ix])[e], nvox)
        dsum = np.bincount(v, wv * O.dgd[ix][e], nvox)
        n = np.bincount(v, minlength=nvox)
    if np.any((n == 0) & (got != 0)):
        raise AssertionError(f'{what}: non-zero where no sample contributes: voxels {np.nonzero((n == 0) & (got != 0))[0][:5]}')
    return _hold(what, got, ref, dsum + gamma(n + 2 + SLACK) * mag + n * TINY)


# ------------------------------------------------------------------------------------------ float32 evaluations (host tests)
def emulate_tree(R, last, gw, g_last, interval, mutant=None):
    """march_density_bwd_kernel's order in numpy float32: chunks of 64 records from the far end, `wave_suffix_excl`'s
    shuffle tree, `acc += total`.  -> g_d [E] float32.  `mutant` (host tests: a wrong evaluation must fail the checks):
    'drop64' the term of record 64 never enters a sum; 'no_eps' no 1e-10 in the denominator; 'T_after' T taken after
    the multiply."""
    E = R.ray.shape[0]
    out = np.zeros(E, np.float32)
    lanes = np.arange(64)
    last = np.asarray(last, np.float32)
    with np.errstate(all='ignore'):
        for r in range(R.n.shape[0]):
            a, n = int(R.first[r]), int(R.n[r])
            if n == 0:
                continue
            T, al, e, g = R.T[a:a + n], R.alpha[a:a + n], R.exp_d[a:a + n], gw[a:a + n]
            if mutant == 'T_after':
                T = R.T_after[a:a + n]
            w = R.T[a:a + n] * al
            acc = (_F(0) if g_last is None else _F(g_last[r])) * last[r]
            for hi in range(n, 0, -64):
                lo = max(0, hi - 64)
                v = np.zeros(64, np.float32)
                v[:hi - lo] = g[lo:hi] * w[lo:hi]
                if mutant == 'drop64' and lo <= 64 < hi:
                    v[64 - lo] = 0
                inc = v.copy()
                for d in (1, 2, 4, 8, 16, 32):
                    sh = np.zeros(64, np.float32)
                    sh[:64 - d] = inc[d:]
                    inc = np.where(lanes + d < 64, inc + sh, inc).astype(np.float32)
                ex = np.concatenate([inc[1:], np.zeros(1, np.float32)])
                my = (acc + ex)[:hi - lo]
                acc = _F(acc + inc[0])
                gt = g[lo:hi] * T[lo:hi]
                om = (_F(1) - al[lo:hi]).astype(np.float64) + (0.0 if mutant == 'no_eps' else 1e-10)
                ga = (gt.astype(np.float64) - my.astype(np.float64) / om).astype(np.float32)
                p = np.power((_F(1) + e[lo:hi]).astype(np.float64), float(-_F(interval) - _F(1))).astype(np.float32)
                v64 = np.minimum(e[lo:hi].astype(np.float64), 1e10) * p.astype(np.float64)
                out[a + lo:a + hi] = (v64 * float(_F(interval)) * ga.astype(np.float64)).astype(np.float32)
    return out


def serial_c_oracle(oracle, R, last, gw, g_last, interval, fma=True):
    """The reference's serial walk: oracle/dvgo_oracle.c alpha2weight_backward (fma or plain) + raw2alpha_backward."""
    N = R.n.shape[0]
    gl = np.zeros(N, np.float32) if g_last is None else np.asarray(g_last, np.float32)
    ga = oracle.alpha2weight_backward(R.alpha, R.w, R.T, np.asarray(last, np.float32), R.first[:-1], R.first[1:], N, gw, gl, fma=fma)
    return oracle.raw2alpha_backward(R.exp_d, ga, float(_F(interval)))


def records_from_alpha(alpha_rays, thres=0.0, exp_d_rays=None, interval=0.5):
    """Records as march_density would leave them for rays whose candidate alphas are given (host tests): the float32
    recurrence, the stop, the flags.  -> (Records, n3, last)"""
    rows, n2, n3, last = [], [], [], []
    for r, al in enumerate(alpha_rays):
        al = np.asarray(al, np.float32)
        T, c2, c3 = _F(1), 0, 0
        for j, a in enumerate(al):
            if thres > 0 and not a > _F(thres):
                continue
            flag = (T * a > _F(thres)) if thres > 0 else True
            with np.errstate(all='ignore'):
                e = (_F(np.float64(1.0 - float(a)) ** (-1.0 / interval) - 1.0)) if exp_d_rays is None else _F(exp_d_rays[r][j])
            rows.append((np.int32(j | (-0x80000000 if flag else 0)).view(np.float32), e, a, T))
            c2, c3 = c2 + 1, c3 + int(flag)
            T = _F(float(T) * (1.0 - float(a) + 1e-10))
            if float(T) < 1e-3:
                break
        n2.append(c2); n3.append(c3); last.append(T)
    rec2 = np.array(rows, np.float32).reshape(-1, 4)
    n2 = np.array(n2, np.int64)
    R = Records(rec2, n2, np.concatenate([[0], np.cumsum(n2)])[:-1])
    return R, np.array(n3, np.int64), np.array(last, np.float32)


# ------------------------------------------------------------------------------------------ the launch spy
_NAMES = ('dvgo_march_density', 'dvgo_march_gather', 'dvgo_march_composite', 'dvgo_march_composite_bwd', 'dvgo_march_density_bwd')
_ORDER = {fn: sorted(ix, key=ix.get) for fn, ix in ((fn, B.param_index(fn)) for fn in _NAMES)}


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


class MarchSpy(B.LaunchSpy):
    """with MarchSpy() as spy: ...  Every launch of the five march entry points issued inside is held to this module when it
    returns.  `report[name]`: one (elements checked, worst err / bound) per launch (exact checks report 0.0).
    `brick=True` also runs `LaunchSpy`'s own check of dvgo_brick_accumulate."""

    def __init__(self, check=True, brick=False):
        super().__init__(check)
        self.brick, self.report, self.seen = brick, {n: [] for n in _NAMES}, {}

    def _call(self, name, *args):
        if name not in _NAMES:
            if self.brick:
                return super()._call(name, *args)
            self.calls.append(name)
            return self._orig(name, *args)
        import torch
        self.calls.append(name)
        if torch.cuda.is_current_stream_capturing():
            return self._orig(name, *args)
        names = _ORDER[name]
        assert len(args) == len(names)
        a = dict(zip(names, args))
        return getattr(self, '_on_' + name[len('dvgo_'):])(name, a, args)

    def _run(self, name, args):
        import torch
        self._orig(name, *args)
        torch.cuda.synchronize()

    def _records(self, a):
        n_steps = _np(a['n_steps'])
        return Records(_np(a['rec2']), _np(a['n2']), rec_base(n_steps, _np(a['n_steps_cumsum']), a['rec_stride'])), n_steps

    def _on_march_density(self, name, a, args):
        self._run(name, args)
        if a['n_rays'] == 0:
            return
        # with rays_o given the records are at ray * rec_stride whatever n_steps_cumsum holds (march.hip: cs0)
        n_steps = _np(a['n_steps'])
        cum = None if a['rays_o'] is not None else _np(a['n_steps_cumsum'])
        R = Records(_np(a['rec2']), _np(a['n2']), rec_base(n_steps, cum, a['rec_stride']))
        E = check_records(R, n_steps, a['fast_color_thres'], _np(a['n3']), _np(a['alphainv_last']))
        self.seen['records'], self.seen['n3'] = R, _np(a['n3']).astype(np.int64)
        self.seen['thres'] = a['fast_color_thres']
        self.seen['n_steps'], self.seen['start'], self.seen['last'] = n_steps, _np(a['rays_start']), _np(a['alphainv_last'])
        self.report[name].append((E, 0.0))

    def _on_march_gather(self, name, a, args):
        self._run(name, args)
        if a['n_rays'] == 0:
            return
        R, _ = self._records(a)
        N = a['n_rays']
        n3 = np.bincount(R.ray, R.flag, N).astype(np.int64)
        M = check_gather(R, n3, _np(a['off3'])[:N + 1], _np(a['ray_id']), _np(a['step_id']), _np(a['weights']), _np(a['alpha']))
        assert M <= a['M3']
        self.report[name].append((M, 0.0))

    def _on_march_composite(self, name, a, args):
        self._run(name, args)
        N = a['n_rays']
        if N == 0:
            return
        off3 = _np(a['off3'])[:N + 1]
        worst = check_composite(_np(a['weights']), _np(a['rgb']), _np(a['step_id']), off3, _np(a['alphainv_last']), a['bg'],
                                _np(a['rgb_marched']), _np(a['depth']))
        self.report[name].append((int(off3[-1]), worst))

    def _on_march_composite_bwd(self, name, a, args):
        import torch
        torch.cuda.synchronize()
        M = a['M3'] if a['m_dev'] is None else min(a['M3'], int(_np(a['m_dev']).reshape(-1)[0]))
        acc = bool(a['accumulate'])
        b_rgb = _np(a['grad_rgb'][:M]).copy() if acc and a['grad_rgb'] is not None else None
        b_last = _np(a['grad_last']).copy() if acc and a['grad_last'] is not None else None
        self._run(name, args)
        worst = check_composite_bwd(_np(a['grad_rgb_marched']), _np(a['weights']), _np(a['rgb']), _np(a['ray_id']), M, a['bg'],
                                    _np(a['grad_weights']), _np(a['grad_rgb']), _np(a['grad_last']), b_rgb, b_last)
        self.report[name].append((M, worst))

    def _on_march_density_bwd(self, name, a, args):
        import torch
        N = a['n_rays']
        if N == 0:
            return self._orig(name, *args)
        torch.cuda.synchronize()
        dims = (a['X'], a['Y'], a['Z'])
        nvox = dims[0] * dims[1] * dims[2]
        dense = None
        if a['brick_cursor'] is None:
            t = a['grad_density']
            dense = torch.as_strided(t, (nvox,), (a['grad_stride'],), t.storage_offset())
            assert not bool(dense.any()), 'grad_density is expected to be zero before the launch'
        self._run(name, args)
        R, _ = self._records(a)
        off3 = _np(a['off3'])[:N + 1]
        gw = gw_per_record(R, off3, _np(a['grad_weights']))
        O = density_bwd_reference(R, _np(a['alphainv_last']), gw, _np(a['grad_last']), a['interval'], 'tree')
        E = R.ray.shape[0]
        if a['brick_cursor'] is not None:
            n_ent = int(a['brick_cursor'].max())
            ent = _np(a['brick_recs'][:n_ent]).reshape(-1, 4).view(np.int32)
            key = R.ray * (1 << 31) + R.step
            ekey = ent[:, 1].astype(np.int64) * (1 << 31) + ent[:, 2]
            pos = np.minimum(np.searchsorted(key, ekey), max(E - 1, 0))
            assert E > 0 or n_ent == 0
            assert np.array_equal(key[pos], ekey), 'a brick-list entry names a (ray, step) that is no record'
            assert np.all(np.bincount(pos, minlength=E) >= 1), 'a record is in no brick list'
            want_kept = np.where(R.flag, off3[R.ray] + R.rank, -1)
            assert np.array_equal(ent[:, 0], want_kept[pos]), 'kept index of a brick-list entry'
            g_d = np.zeros(E, np.float32)
            g_d.view(np.int32)[pos] = ent[:, 3]
            assert np.array_equal(g_d.view(np.int32)[pos], ent[:, 3]), 'the entries of one sample differ in g_d'
            worst = check_density_bwd(R, O, g_d)
            self.report[name].append((E, worst, n_ent))
        else:
            kept = _np(a['grad_kept'])
            direct = R.flag if kept is not None else np.zeros(E, bool)
            worst = 0.0
            if direct.any():
                g_d = np.zeros(E, np.float32)
                g_d[direct] = kept[off3[R.ray[direct]] + R.rank[direct]]
                Od = _subset(O, direct)
                worst = check_density_bwd(_SubRecords(R, direct), Od, g_d[direct], 'march_density_bwd grad_kept')
            ws = check_density_scatter(R, O, ~direct, _np(a['rays_start']), _np(a['rays_dir']), a['stepdist'],
                                       np.array(list(a['xyz_min']), np.float32), np.array(list(a['xyz_max']), np.float32), dims, _np(dense))
            self.report[name].append((E, max(worst, ws), int(direct.sum())))


    def summary(self):
        """{entry point: (launches, elements checked, worst err / bound)}"""
        return {n[len('dvgo_'):]: (len(v), sum(x[0] for x in v), round(max((x[1] for x in v), default=0.0), 4)) for n, v in self.report.items()}


class _SubRecords:
    def __init__(self, R, sel):
        self.n = R.n
        for k in ('ray', 'idx', 'step', 'alpha', 'T', 'exp_d'):
            setattr(self, k, getattr(R, k)[sel])


def _subset(O, sel):
    S = DensityBwdRef()
    for k in ('ga', 'dga', 'gd', 'dgd', 'zero'):
        setattr(S, k, getattr(O, k)[sel])
    return S
