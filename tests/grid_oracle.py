"""Float64 statement of the op-by-op trilinear family and of the per-ray sum (test infrastructure, CPU only, numpy).

It covers `dvgo_grid_sample_fwd` / `dvgo_grid_sample_bwd` (csrc/grid_sample.hip), `dvgo_view_weight_accumulate` /
`dvgo_view_count_commit` (csrc/maintain.hip) and `dvgo_segment_sum` (csrc/composite.hip).  The float32 trilinear setup,
`fma32`, `gamma`, U, SLACK, TINY, `scatter(by_sample=True)` and `check_dense` are tests/brick_oracle.py's, which
tests/test_brick_oracle_host.py pins to oracle/dvgo_oracle.c; nothing of them is restated here.

a. Gather.  The expected values are the C oracle's `grid_sample_fwd(use_fma=True)`, bit for bit: the kernels run the
   same eight `fmaf` in the same corner order per channel, in either layout and on either dispatch branch.

b. Scatter.  Per voxel and channel, ref = sum w g, mag = sum |w g|, n = number of in-range corners that reach the voxel
   (`scatter(by_sample=True)`).  Both backward kernels round each product once (`w * g`) and add it to memory with a
   float atomic, in any order: `check_dense(atomic=True)`, |got - ref| <= gamma(n + 2 + SLACK) mag + (n + 1) TINY, and an
   exact 0.0 where mag == 0.  A pre-filled `grad_grid` enters as one more term of every element (ref += v, mag += |v|,
   n += 1): it passes the n additions of the chain like any other term and carries no product rounding.

c. View weights (`view_weight_kernel`).  The sample positions are inputs of the sum, not part of what is bounded; they
   are restated in numpy float32 operation for operation, without contraction (the library is built with
   -ffp-contract=off): v = d, or 1e-6f where d == 0; the six quotients (max - o) / v, (min - o) / v;
   t_min = fmax(fmax(fmin(ax, bx), fmin(ay, by)), fmin(az, bz)), then fmin(fmax(t_min, near), far);
   norm = sqrt((dx dx + dy dy) + dz dz); t = t_min + (step * (float)k) / norm; p = o + d * t (product and sum rounded
   separately).  The trilinear setup of p is brick_oracle.tri_setup.  Per voxel, in float64:
       ref = sum w      mag = sum |w|      n = number of in-range corners of the view's samples that reach the voxel.
   Bound.  A weight is a float32 number and enters the sum unrounded (there is no product).  The kernel adds the weights
   of one wavefront pass (64 samples of one ray) that share a voxel into one slot of the wave's table (`atomicAdd` on
   LDS, the slot starts at 0.0f: k_t additions for k_t weights), then adds each occupied slot to `acc` (one float atomic
   per slot); a weight whose key found no slot within 16 probes goes to `acc` directly, which is a table of one weight
   and no table addition.  So a weight passes at most k_t additions in its table and at most T additions in memory,
   T the number of tables (and direct additions) that reach the voxel.  Every other table holds at least one weight:
   k_t + (T - 1) <= n, k_t + T <= n + 1, and
       |got - ref| <= gamma(n + 1 + SLACK) mag + n TINY.
   SLACK = 1 covers the float64 evaluation of ref; n TINY is kept for symmetry with the scatter (float additions carry
   no underflow error).  Where n == 0, `acc` stays exactly 0.0.  No constant was fitted to GPU output.

d. Count rule (`view_commit_kernel`: count += acc > 1).  A voxel is counted if ref - 1 > bound, not counted if
   1 - ref > bound, undetermined otherwise; only undetermined voxels may go either way.

e. Segment sum.  Per (segment, channel), ref, mag and n include `out`'s initial value as one term (n = rows + 1).  The
   kernel sums the rows of a segment that share a wavefront in a Hillis-Steele tree and adds every tail to `out` with
   an atomic: some summation order of n terms, n - 1 additions, |got - ref| <= gamma(n - 1 + SLACK) mag.  A segment
   without rows keeps `out` bit for bit.

f. Hash.  `hash_home`, `place` and `overflow_certificate` restate the table's addressing -- (key * 2654435761 mod 2^32)
   >> 23, linear probing over 16 of 512 slots -- only to show ON THE CPU that an input cannot fit whatever the
   insertion order; they are never compared with device memory.
"""
import numpy as np

import brick_oracle as B
from brick_oracle import SLACK, TINY, gamma

_F = np.float32
TABLE, PROBES = 512, 16


# ------------------------------------------------------------------------------------------ a. gather
def gather(oracle, grid, xyz, xyz_min, xyz_max):
    """grid [C, X, Y, Z] numpy (any strides) -> [M, C]: the C oracle's fused-multiply-add chain."""
    return oracle.grid_sample_fwd(grid, xyz, xyz_min, xyz_max, use_fma=True)


# ------------------------------------------------------------------------------------------ b. scatter
def scatter_sums(xyz, grad_out, xyz_min, xyz_max, dims, prefill=None):
    """The sums of one dvgo_grid_sample_bwd: xyz [M, 3], grad_out [M, C]; `prefill` [C, X, Y, Z]: what grad_grid held."""
    X, Y, Z = dims
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    M = xyz.shape[0]
    grad_out = np.asarray(grad_out, np.float32).reshape(M, -1)
    C = grad_out.shape[1]
    recs = np.zeros((M, 4), np.int32)
    recs[:, 0] = recs[:, 1] = np.arange(M)                       # kept index and "ray": the position is rays_start
    O = B.scatter(recs, None, xyz, np.zeros_like(xyz), 0.5, xyz_min, xyz_max, grad_out, C, X, Y, Z, by_sample=True)
    if prefill is not None:
        pre = np.moveaxis(np.asarray(prefill, np.float64).reshape(C, X, Y, Z), 0, -1).reshape(-1, C)
        O.ref[:, :C] += pre
        O.mag[:, :C] += np.abs(pre)
        O.n = O.n + 1
    return O


def check_scatter(O, grad, what='grid_sample backward'):
    """grad [C, X, Y, Z] numpy float32 (any strides).  -> worst err / bound"""
    X, Y, Z, C = O.shape
    grad = np.ascontiguousarray(np.asarray(grad).reshape(C, X, Y, Z))
    return B.check_dense(O, grad, np.zeros((X, Y, Z), np.float32), atomic=True, what=what)


# ------------------------------------------------------------------------------------------ c. view weights
def view_positions(rays_o, rays_d, xyz_min, xyz_max, near, far, step, n_samples):
    """[R, n_samples, 3] float32 sample positions of view_weight_kernel, operation for operation."""
    o = np.asarray(rays_o, np.float32).reshape(-1, 3)
    d = np.asarray(rays_d, np.float32).reshape(-1, 3)
    mn, mx = np.asarray(xyz_min, np.float32), np.asarray(xyz_max, np.float32)
    near, far, step = _F(near), _F(far), _F(step)
    with np.errstate(all='ignore'):
        v = np.where(d == 0, _F(1e-6), d).astype(np.float32)
        a, b = (mx - o) / v, (mn - o) / v
        lo = np.fmin(a, b)
        t_min = np.fmax(np.fmax(lo[:, 0], lo[:, 1]), lo[:, 2])
        t_min = np.fmin(np.fmax(t_min, near), far)
        sq = d * d
        norm = np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2])
        k = np.arange(n_samples, dtype=np.int64).astype(np.float32)
        t = t_min[:, None] + (step * k)[None, :] / norm[:, None]
        p = o[:, None, :] + d[:, None, :] * t[:, :, None]
    assert p.dtype == np.float32
    return p


class ViewSums:
    """ref, mag [n_vox] float64, n [n_vox] of one view."""

    def __init__(self, ref, mag, n, dims):
        self.ref, self.mag, self.n, self.dims = ref, mag, n, dims

    def bound(self):
        return gamma(self.n + 1 + SLACK) * self.mag + self.n * TINY


def view_terms(pos, xyz_min, xyz_max, dims):
    """-> (sample index, voxel, weight float32) of every in-range corner, by sample then corner"""
    X, Y, Z = dims
    _, w, inb, vox = B.tri_setup(np.asarray(pos, np.float32).reshape(-1, 3), xyz_min, xyz_max, X, Y, Z)
    e, q = np.nonzero(inb)
    return e, vox[e, q], w[e, q]


def view_sums(pos, xyz_min, xyz_max, dims):
    nvox = int(np.prod(dims))
    _, v, w = view_terms(pos, xyz_min, xyz_max, dims)
    w = w.astype(np.float64)
    return ViewSums(np.bincount(v, weights=w, minlength=nvox), np.bincount(v, weights=np.abs(w), minlength=nvox),
                    np.bincount(v, minlength=nvox), tuple(dims))


def _fail(name, bad, *cols):
    idx = np.argwhere(bad)[:5]
    rows = [tuple(int(i) for i in ix) + tuple(float(c[tuple(ix)]) for c in cols) for ix in idx]
    raise AssertionError(f'{name}: {int(bad.sum())} of {bad.size} elements; first (index..., values...): {rows}')


def check_view(V, acc, what='view weights'):
    """acc [n_vox] float32 before any commit.  -> worst err / bound"""
    got = np.asarray(acc, np.float32).reshape(-1).astype(np.float64)
    if not np.all(np.isfinite(got)):
        _fail(f'{what}: non-finite sum', ~np.isfinite(got), got)
    zero = V.n == 0
    if np.any(zero & (got != 0)):
        _fail(f'{what}: weight on a voxel no sample reaches', zero & (got != 0), got)
    err, bound = np.abs(got - V.ref), V.bound()
    if np.any(err > bound):
        _fail(f'{what}: sum outside gamma(n + 1 + {SLACK}) * mag', err > bound, got, V.ref, V.mag, V.n)
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.where(bound > 0, err / bound, 0.0)
    return float(r.max()) if r.size else 0.0


# ------------------------------------------------------------------------------------------ d. count rule
def count_rule(V):
    """-> (counted, not_counted, undetermined) bool [n_vox]"""
    b = V.bound()
    counted, not_counted = (V.ref - 1.0) > b, (1.0 - V.ref) > b
    return counted, not_counted, ~(counted | not_counted)


def undetermined_share(V):
    """undetermined voxels over the voxels with ref > 0"""
    return float(count_rule(V)[2].sum()) / max(int((V.ref > 0).sum()), 1)


def check_counts(views, count, what='view count', max_share=0.01):
    """views: the ViewSums of the views in order; count [n_vox] after all commits.  Every determined voxel exact: the
    count lies in [sum counted, sum counted + sum undetermined] and is an integer; per view at most `max_share`
    undetermined."""
    got = np.asarray(count, np.float64).reshape(-1)
    lo, und = np.zeros(got.shape[0]), np.zeros(got.shape[0])
    for i, V in enumerate(views):
        c, _, u = count_rule(V)
        share = undetermined_share(V)
        assert share <= max_share, f'{what}: view {i}: {share:.4f} of the voxels with ref > 0 are undetermined'
        lo += c
        und += u
    bad = (got < lo) | (got > lo + und) | (got != np.round(got))
    if np.any(bad):
        _fail(f'{what}: count outside what the determined views fix', bad, got, lo, und)
    return int(und.sum())


# ------------------------------------------------------------------------------------------ e. segment sum
class SegSums:
    def __init__(self, ref, mag, n, rows):
        self.ref, self.mag, self.n, self.rows = ref, mag, n, rows

    def bound(self):
        return gamma(self.n - 1 + SLACK)[:, None] * self.mag


def segment_sums(src, index, out0):
    """src [M, C] (or [M]), index [M] sorted, out0 [N, C] (or [N]): out's value before the launch."""
    index = np.asarray(index, np.int64)
    out0 = np.asarray(out0, np.float32)
    N = out0.shape[0]
    out0 = out0.reshape(N, -1).astype(np.float64)
    C = out0.shape[1]
    src = np.asarray(src, np.float32).reshape(-1, C).astype(np.float64)
    assert src.shape[0] == index.shape[0] and np.all(np.diff(index) >= 0) and (index.size == 0 or (index[0] >= 0 and index[-1] < N))
    ref, mag = out0.copy(), np.abs(out0)
    for c in range(C):
        ref[:, c] += np.bincount(index, weights=src[:, c], minlength=N)
        mag[:, c] += np.bincount(index, weights=np.abs(src[:, c]), minlength=N)
    rows = np.bincount(index, minlength=N)
    return SegSums(ref, mag, rows + 1, rows)


def check_segment(S, got, out0, what='segment_sum'):
    """-> worst err / bound"""
    N = S.rows.shape[0]
    got32 = np.asarray(got, np.float32).reshape(N, -1)
    out0 = np.asarray(out0, np.float32).reshape(N, -1)
    got = got32.astype(np.float64)
    if not np.all(np.isfinite(got)):
        _fail(f'{what}: non-finite sum', ~np.isfinite(got), got)
    keep = (S.rows == 0)[:, None] & (got32.view(np.int32) != out0.view(np.int32))
    if np.any(keep):
        _fail(f'{what}: a segment without rows changed', keep, got, out0.astype(np.float64))
    err, bound = np.abs(got - S.ref), S.bound()
    if np.any(err > bound):
        _fail(f'{what}: sum outside gamma(n - 1 + {SLACK}) * mag', err > bound, got, S.ref, S.mag, np.broadcast_to(S.n[:, None], got.shape))
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.where(bound > 0, err / bound, 0.0)
    return float(r.max()) if r.size else 0.0


# ------------------------------------------------------------------------------------------ f. the table's hash
def hash_home(keys):
    keys = np.asarray(keys, np.int64).astype(np.uint64)
    return (((keys * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(23)).astype(np.int64)


def place(keys):
    """Insert `keys` (repeats allowed) in the given order.  -> placed [len(keys)] bool"""
    slots = np.full(TABLE, -1, np.int64)
    placed = np.zeros(len(keys), bool)
    for i, (k, h) in enumerate(zip(np.asarray(keys, np.int64), hash_home(keys))):
        for p in range(PROBES):
            s = (h + p) % TABLE
            if slots[s] == -1 or slots[s] == k:
                slots[s] = k
                placed[i] = True
                break
    return placed


def overflow_certificate(keys):
    """A circular slot range [a, a + L) that more distinct keys have their whole 16-slot window inside than it has slots:
    at least one of them finds no slot in ANY insertion order (each placed key holds a slot of its own window).
    -> (a, L, keys inside) or None.  More than 512 distinct keys is the range of the whole table."""
    keys = np.unique(np.asarray(keys, np.int64))
    if keys.size > TABLE:
        return 0, TABLE, int(keys.size)
    hist = np.bincount(hash_home(keys), minlength=TABLE)
    cum = np.concatenate([[0], np.cumsum(np.concatenate([hist, hist]))])
    best = None
    for L in range(PROBES, TABLE):
        span = L - PROBES + 1                                   # homes a .. a + L - 16 have their window inside
        inside = cum[np.arange(TABLE) + span] - cum[np.arange(TABLE)]
        a = int(np.argmax(inside))
        if inside[a] > L and (best is None or inside[a] - L > best[2] - best[1]):
            best = (a, L, int(inside[a]))
    return best


def chunk_keys(pos, xyz_min, xyz_max, dims, chunk):
    """The keys (flat voxel indices, repeats included) that the samples [64 chunk, 64 chunk + 64) of ONE ray insert."""
    e, v, _ = view_terms(pos, xyz_min, xyz_max, dims)
    return v[(e >= 64 * chunk) & (e < 64 * chunk + 64)]
