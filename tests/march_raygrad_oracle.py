"""Float64 statement of `dvgo_march_ray_bwd` (csrc/march.hip): the gradient of the fused march with respect to its rays.
Test infrastructure, CPU only, numpy.  It is assembled from two oracles that exist and adds no constant of its own:

  g_d     per record, `march_oracle.density_bwd_reference` (order 'tree': the kernel walks the records as march_density_bwd
          does): reference O.gd and bound O.dgd;
  nabla   per record, `raygrad_oracle.sums` on the record's float32 position p = fmaf(rays_dir, dist, rays_start)
          (`brick_oracle.positions`) with the cell and the float32 per-axis weights as INPUTS (`raygrad_oracle.inputs32`):
          S1 = the density grid's position derivative (grad_out = 1), Sf = the feature grid's with the record's grad_feat row
          (records kept by march_gather, when grad_feat is given; zero rows elsewhere).

Per record the kernel continues ONE chain over C' + 1 channels -- the density grid with g_d, then the C' feature channels (C' = C
for a record with a feature term, else 0) -- so with k = (C' + 1) + 12 + SLACK of raygrad_oracle's count
    ref_p   = gd * S1.ref + Sf.ref
    bound_p = dgd * |S1.ref| + gamma(k) * ((|gd| + dgd) * S1.mag + Sf.mag) + tiny
i.e. bound(g_d) |nabla| + |g_d| bound(nabla): the first term is what the kernel's g_d may differ by, the second the rounding of
the chain on the magnitudes the kernel can hold; tiny is raygrad_oracle's underflow allowance at those magnitudes.

lam = t_min + dist / |d|.  t_min is the sampler's float32 value, an INPUT (a constant of the derivative: INTEGRATION.md section
7, and a min / max over box faces).  dist = stepdist * step and |d| are taken in float64 from the float32 stepdist and rays_d.
The kernel rounds dist once, |d| four times (dx * dx, two fmaf, sqrtf), the division once and the addition once:
    |lam32 - lam| <= dlam = gamma(7 + SLACK) (|t_min| + dist / |d|).

Per ray of n records: A = sum ref_p, B = sum lam ref_p.  A term of B is one more float32 product:
    tb = (|lam| bound_p + dlam (|ref_p| + bound_p)) (1 + u) + u |lam ref_p| + TINY
and the sums are float32 in a fixed tree (a butterfly per chunk of 64, chunks far to near; adding the exact zeros of lanes
without a record rounds nothing): n terms, in the manner of `grid_oracle.segment_sums`,
    |grad_o - A| <= sum bound_p + gamma(n - 1 + SLACK) sum (|ref_p| + bound_p) + n TINY
    |grad_d - B| <= sum tb      + gamma(n - 1 + SLACK) sum (|lam ref_p| + tb)  + n TINY.
A ray without records must be exact zeros.  A ray is `finite` unless `density_bwd_reference` is itself non-finite for one of its
records (exp_d = inf, alpha == 1 with acc != 0: 0 * inf or x / 1e-10 beyond float32); the tests name those rays.
"""
import numpy as np

import brick_oracle as B
import march_oracle as M
import raygrad_oracle as RG
from brick_oracle import SLACK, TINY, U, gamma

_F = np.float32


class RayGrad:
    """A, B [N,3] references; magA, magB their magnitude sums; boundA, boundB; n [N] records per ray; finite [N];
    per record: ref_p, bound_p [E,3], lam, dlam [E], gd (O.gd)"""


def record_positions(Rc, rays_start, rays_dir, stepdist):
    recs = np.stack([np.zeros_like(Rc.step), Rc.ray, Rc.step, np.zeros_like(Rc.step)], 1).astype(np.int64)
    return B.positions(recs, np.asarray(rays_start, np.float32).reshape(-1, 3), np.asarray(rays_dir, np.float32).reshape(-1, 3), stepdist)


def lam_reference(Rc, t_min, rays_d, stepdist):
    """-> (lam [E] float64, dlam [E])"""
    t = np.asarray(t_min, np.float32).astype(np.float64)[Rc.ray]
    d = np.asarray(rays_d, np.float32).astype(np.float64).reshape(-1, 3)
    q = float(_F(stepdist)) * Rc.step.astype(np.float64) / np.sqrt((d * d).sum(-1))[Rc.ray]
    return t + q, gamma(7 + SLACK) * (np.abs(t) + q)


def feat_rows(Rc, off3, grad_feat, C):
    """[E,C] float64: grad_feat[off3[r] + rank] for the flagged records, zero rows elsewhere"""
    g = np.zeros((Rc.ray.shape[0], C))
    k = Rc.flag
    if k.any():
        g[k] = np.asarray(grad_feat, np.float64).reshape(-1, C)[np.asarray(off3, np.int64)[Rc.ray[k]] + Rc.rank[k]]
    return g


def _per_ray(Rc, x):
    N = Rc.n.shape[0]
    out = np.zeros((N, x.shape[1]))
    for c in range(x.shape[1]):
        with np.errstate(invalid='ignore'):
            out[:, c] = np.bincount(Rc.ray, x[:, c], N)
    return out


def reference(Rc, last, gw, g_last, interval, rays_start, rays_dir, stepdist, xyz_min, xyz_max, density, k0, gfeat, t_min, rays_d):
    """Rc: march_oracle.Records; gw [E] upstream gradient per record (`march_oracle.gw_per_record`), g_last [N] or None;
    density [X,Y,Z]; k0 [C,X,Y,Z] and gfeat [E,C] (`feat_rows`), or both None: no feature term.  -> RayGrad"""
    density = np.asarray(density)
    dims = density.shape
    E = Rc.ray.shape[0]
    O = M.density_bwd_reference(Rc, last, gw, g_last, interval, 'tree')
    p = record_positions(Rc, rays_start, rays_dir, stepdist)
    I = RG.inputs32(p, xyz_min, xyz_max, dims)
    s = RG.scale(xyz_min, xyz_max, dims)
    G = RayGrad()
    with np.errstate(all='ignore'):
        S1 = RG.sums(density[None], np.ones((E, 1)), I, s)
        hi = RG.sums(density[None], (np.abs(O.gd) + O.dgd)[:, None], I, s)          # its mag and tiny: at what the kernel may hold
        ref_p = O.gd[:, None] * S1.ref
        mag, tiny = hi.mag, hi.tiny
        Cf = np.zeros(E, np.int64)
        if k0 is not None and np.asarray(k0).shape[0] > 0:
            Sf = RG.sums(k0, gfeat, I, s)
            ref_p, mag, tiny = ref_p + Sf.ref, mag + Sf.mag, tiny + Sf.tiny
            Cf = np.where(Rc.flag, np.asarray(k0).shape[0], 0)
        k = Cf + 1 + 12 + SLACK
        bound_p = O.dgd[:, None] * np.abs(S1.ref) + gamma(k)[:, None] * mag + tiny
        lam, dlam = lam_reference(Rc, t_min, rays_d, stepdist)
        ref_b = lam[:, None] * ref_p
        tb = (np.abs(lam)[:, None] * bound_p + dlam[:, None] * (np.abs(ref_p) + bound_p)) * (1 + U) + U * np.abs(ref_b) + TINY
        n = Rc.n
        gs = gamma(np.maximum(n - 1, 0) + SLACK)[:, None]
        G.A, G.B = _per_ray(Rc, ref_p), _per_ray(Rc, ref_b)
        G.magA, G.magB = _per_ray(Rc, np.abs(ref_p)), _per_ray(Rc, np.abs(ref_b))
        G.boundA = _per_ray(Rc, bound_p) + gs * _per_ray(Rc, np.abs(ref_p) + bound_p) + (n * TINY)[:, None]
        G.boundB = _per_ray(Rc, tb) + gs * _per_ray(Rc, np.abs(ref_b) + tb) + (n * TINY)[:, None]
    bad = ~(np.isfinite(O.gd) & np.isfinite(O.dgd))
    G.finite = np.bincount(Rc.ray, bad, n.shape[0]) == 0
    G.n, G.ref_p, G.bound_p, G.lam, G.dlam, G.gd = n, ref_p, bound_p, lam, dlam, O.gd
    return G


def check(G, grad_o, grad_d, excluded=(), what='march_ray_bwd'):
    """grad_o, grad_d [N,3] float32.  `excluded`: the rays the caller names as having no finite reference -- exactly the rays
    with G.finite False, or the check fails.  -> worst err / bound over the other rays"""
    N = G.n.shape[0]
    got = [np.asarray(x, np.float32).reshape(N, 3) for x in (grad_o, grad_d)]
    assert sorted(int(r) for r in excluded) == np.nonzero(~G.finite)[0].tolist(), (f'{what}: rays without a finite reference', np.nonzero(~G.finite)[0].tolist(), sorted(excluded))
    ok = G.finite
    worst = 0.0
    for name, g32, ref, bound in (('grad_o', got[0], G.A, G.boundA), ('grad_d', got[1], G.B, G.boundB)):
        g = g32.astype(np.float64)
        assert np.all(np.isfinite(g[ok])), (f'{what}: {name} non-finite (unwritten?)', np.argwhere(~np.isfinite(g) & ok[:, None])[:5].tolist())
        empty = G.n == 0
        assert not g32[empty].any(), f'{what}: {name} of a ray without records is not exact zeros'
        err = np.abs(g - ref)
        bad = ok[:, None] & ~(err <= bound)
        if bad.any():
            ix = np.argwhere(bad)[:5]
            rows = [(tuple(int(v) for v in i), int(G.n[i[0]]), float(g[tuple(i)]), float(ref[tuple(i)]), float(err[tuple(i)]), float(bound[tuple(i)])) for i in ix]
            raise AssertionError(f'{what}: {name}: {int(bad.sum())} of {int(ok.sum()) * 3} outside the bound; first ((ray, axis), records, got, ref, err, bound): {rows}')
        with np.errstate(invalid='ignore', divide='ignore'):
            r = np.where(bound[ok] > 0, err[ok] / bound[ok], 0.0)
        worst = max(worst, float(r.max()) if r.size else 0.0)
    return worst
