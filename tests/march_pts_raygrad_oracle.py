"""Float64 statement of `dvgo_march_ray_bwd_pts` and `dvgo_march_vm_ray_bwd` (csrc/march_raygrad.hip): the ray gradient
of the fused marches that hand positions to their caller.  Test infrastructure, CPU only, numpy.  It adds no constant of its
own and composes what exists:

  dense entry   per record `march_raygrad_oracle.reference(..., k0=None, gfeat=None)`: ref_p = gd * nabla(density), bound_p;
  VM entry      g_d and its bound from `march_oracle.density_bwd_reference` (order 'tree': the kernel walks the records as
                march_vm_density_bwd does), nabla from `vm_raygrad_oracle.sums` (the density entry) on the record's float32
                position p = fmaf(rays_dir, dist, rays_start): S1 at grad_out = 1 for the reference, `hi` at |g_d| + dgd for the
                magnitudes the kernel may hold, as `march_raygrad_oracle.reference` does with `raygrad_oracle.sums`:
                    ref_p   = gd * S1.ref
                    bound_p = dgd * |S1.ref| + gamma(R + 12 + SLACK) * hi.mag + hi.tiny
                (bound(g_d) |nabla| + the rounding of vm_raygrad_oracle's chain of R + 12 operations at those magnitudes);
  pts term      a record that survived into the M3 arrays adds its row q of grad_pts (`march_raygrad_oracle.feat_rows`, C = 3;
                zero rows elsewhere and when grad_pts is NULL) with ONE float32 addition per component.  The addition rounds
                what the kernel holds, which is within bound_p of ref_p:
                    ref_p'   = ref_p + q
                    bound_p' = bound_p + U * (|ref_p| + bound_p + |q|)        (an addition is exact when its result is
                                                                             subnormal: no TINY)
                A record without the term keeps (ref_p, bound_p): the kernel adds nothing there.

lam, dlam: `march_raygrad_oracle.lam_reference`.  The per-ray sums and their bounds are `march_raygrad_oracle.reference`'s,
term for term (`_finish` restates those lines on the new per-record values; `check` is that module's).  A ray is finite unless
`density_bwd_reference` is non-finite for one of its records.

`evaluate32`: the kernels' float32 arithmetic in their order, in numpy -- `march_oracle.emulate_tree` for g_d, `raygrad_oracle.
evaluate32` / `vm_raygrad_oracle.evaluate32` for nabla (grad_out = g_d: the first product of either chain), the pts addition,
lam as the kernel rounds it, and the xor butterfly per chunk of 64 from the far end.  Its `mutant` argument plants the mistakes
tests/test_march_pts_raygrad_host.py expects the bound to catch.
"""
import numpy as np

import brick_oracle as B
import march_oracle as M
import march_raygrad_oracle as MR
import raygrad_oracle as RG
import vm_raygrad_oracle as VR
from brick_oracle import SLACK, TINY, U, gamma

_F = np.float32
check = MR.check


def pts_rows(Rc, off3, grad_pts):
    """[E,3] float64: grad_pts[off3[r] + rank] for the flagged records, zero rows elsewhere; None stays None"""
    return None if grad_pts is None else MR.feat_rows(Rc, off3, grad_pts, 3)


def _add_pts(Rc, ref_p, bound_p, q):
    if q is None:
        return ref_p, bound_p
    k = Rc.flag[:, None]
    with np.errstate(all='ignore'):
        return (np.where(k, ref_p + q, ref_p),
                np.where(k, bound_p + U * (np.abs(ref_p) + bound_p + np.abs(q)), bound_p))


def _finish(Rc, O, ref_p, bound_p, lam, dlam):
    """march_raygrad_oracle.reference from `ref_b` on"""
    G = MR.RayGrad()
    with np.errstate(all='ignore'):
        ref_b = lam[:, None] * ref_p
        tb = (np.abs(lam)[:, None] * bound_p + dlam[:, None] * (np.abs(ref_p) + bound_p)) * (1 + U) + U * np.abs(ref_b) + TINY
        n = Rc.n
        gs = gamma(np.maximum(n - 1, 0) + SLACK)[:, None]
        G.A, G.B = MR._per_ray(Rc, ref_p), MR._per_ray(Rc, ref_b)
        G.magA, G.magB = MR._per_ray(Rc, np.abs(ref_p)), MR._per_ray(Rc, np.abs(ref_b))
        G.boundA = MR._per_ray(Rc, bound_p) + gs * MR._per_ray(Rc, np.abs(ref_p) + bound_p) + (n * TINY)[:, None]
        G.boundB = MR._per_ray(Rc, tb) + gs * MR._per_ray(Rc, np.abs(ref_b) + tb) + (n * TINY)[:, None]
    bad = ~(np.isfinite(O.gd) & np.isfinite(O.dgd))
    G.finite = np.bincount(Rc.ray, bad, n.shape[0]) == 0
    G.n, G.ref_p, G.bound_p, G.lam, G.dlam, G.gd = n, ref_p, bound_p, lam, dlam, O.gd
    return G


def reference_dense(Rc, last, gw, g_last, interval, rays_start, rays_dir, stepdist, xyz_min, xyz_max, density, gpts, t_min, rays_d):
    """gpts [E,3] (`pts_rows`) or None.  -> march_raygrad_oracle.RayGrad"""
    G0 = MR.reference(Rc, last, gw, g_last, interval, rays_start, rays_dir, stepdist, xyz_min, xyz_max, density, None, None, t_min,
                      rays_d)
    O = M.density_bwd_reference(Rc, last, gw, g_last, interval, 'tree')
    ref_p, bound_p = _add_pts(Rc, G0.ref_p, G0.bound_p, gpts)
    return _finish(Rc, O, ref_p, bound_p, G0.lam, G0.dlam)


def reference_vm(Rc, last, gw, g_last, interval, rays_start, rays_dir, stepdist, xyz_min, xyz_max, planes, lines, gpts, t_min, rays_d):
    """planes / lines: dicts of [1,R,H,W] / [1,R,N,1] float32 arrays.  -> march_raygrad_oracle.RayGrad"""
    E = Rc.ray.shape[0]
    O = M.density_bwd_reference(Rc, last, gw, g_last, interval, 'tree')
    p = MR.record_positions(Rc, rays_start, rays_dir, stepdist)
    with np.errstate(all='ignore'):
        S1 = VR.sums(planes, lines, np.ones(E), p, xyz_min, xyz_max)
        hi = VR.sums(planes, lines, np.abs(O.gd) + O.dgd, p, xyz_min, xyz_max)
        ref_p = O.gd[:, None] * S1.ref
        bound_p = O.dgd[:, None] * np.abs(S1.ref) + gamma(S1.k() + SLACK) * hi.mag + hi.tiny
    ref_p, bound_p = _add_pts(Rc, ref_p, bound_p, gpts)
    lam, dlam = MR.lam_reference(Rc, t_min, rays_d, stepdist)
    return _finish(Rc, O, ref_p, bound_p, lam, dlam)


# ------------------------------------------------------------------------------------------ float32 evaluation (host tests)
MUTANTS = ('no_pts', 'pts_everywhere', 'lam_without_tmin', 'swap_axes', 'no_scale')


def _butterfly(v):
    """wave_sum: v += shfl_xor(v, d) for d = 32 .. 1, float32; -> lane 0"""
    v = np.asarray(v, np.float32).copy()
    lanes = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        v = (v + v[lanes ^ d]).astype(np.float32)
    return v[0]


def evaluate32(Rc, last, gw, g_last, interval, rays_start, rays_dir, stepdist, xyz_min, xyz_max, gpts, t_min, rays_d,
               density=None, planes=None, lines=None, mutant=None, gpts_all=None):
    """-> grad_o, grad_d [N,3] float32.  `density` [X,Y,Z]: the dense entry; `planes`, `lines`: the VM entry.  `mutant`: one of
    MUTANTS ('pts_everywhere' reads `gpts_all` [E,3], rows for the unflagged records too; 'swap_axes' swaps the two world axes of
    plane xy -- of the density's y and z chains in the dense entry; 'no_scale' omits the per-plane / per-axis scale)."""
    assert mutant is None or mutant in MUTANTS
    N, E = Rc.n.shape[0], Rc.ray.shape[0]
    mn, mx = np.asarray(xyz_min, np.float32), np.asarray(xyz_max, np.float32)
    gd = M.emulate_tree(Rc, last, np.asarray(gw, np.float32), g_last, interval)
    p = MR.record_positions(Rc, rays_start, rays_dir, stepdist)
    with np.errstate(all='ignore'):
        if density is not None:
            dims = np.asarray(density).shape
            I = RG.inputs32(p, mn, mx, dims)
            g = RG.evaluate32(np.asarray(density, np.float32)[None], gd[:, None], I, mn, mx, dims, no_scale=mutant == 'no_scale')
            if mutant == 'swap_axes':
                g = g[:, [0, 2, 1]]
        elif mutant == 'swap_axes':
            # plane xy alone with its two axes swapped, then yz and zx: a plane of zeros contributes exact zeros, so each call
            # returns one plane's three terms and the sum below is the kernel's ox = (0 + xy) + yz + zx
            g = np.zeros((E, 3), np.float32)
            for key in VR.KEYS:
                only = {k: (planes[k] if k == key else np.zeros_like(planes[k])) for k in VR.KEYS}
                g = (g + VR.evaluate32(only, lines, gd, p, mn, mx, flip='hw' if key == 'xy' else None)).astype(np.float32)
        else:
            g = VR.evaluate32(planes, lines, gd, p, mn, mx, no_scale=mutant == 'no_scale')
        g = np.where((gd != 0)[:, None], g, _F(0)).astype(np.float32)          # a record with g_d == 0 is passed over
        q = gpts_all if mutant == 'pts_everywhere' else gpts
        if q is not None and mutant != 'no_pts':
            k = np.ones(E, bool) if mutant == 'pts_everywhere' else Rc.flag
            g = np.where(k[:, None], (g + np.asarray(q, np.float32)).astype(np.float32), g)
        d = np.asarray(rays_d, np.float32).reshape(-1, 3)
        rnorm = np.sqrt(B.fma32(d[:, 2], d[:, 2], B.fma32(d[:, 1], d[:, 1], (d[:, 0] * d[:, 0]).astype(np.float32)))).astype(np.float32)
        dist = B.march_dist(stepdist, Rc.step).astype(np.float32)
        t = np.zeros(N, np.float32) if mutant == 'lam_without_tmin' else np.asarray(t_min, np.float32)
        lam = (t[Rc.ray] + (dist / rnorm[Rc.ray]).astype(np.float32)).astype(np.float32)
        has_pts = q is not None and mutant != 'no_pts'
        live = (gd != 0) | ((np.ones(E, bool) if mutant == 'pts_everywhere' else Rc.flag) & has_pts)
        lam = np.where(live, lam, _F(0))
        lg = (lam[:, None] * g).astype(np.float32)
        go, gdir = np.zeros((N, 3), np.float32), np.zeros((N, 3), np.float32)
        for r in range(N):
            a, n = int(Rc.first[r]), int(Rc.n[r])
            for hi in range(n, 0, -64):
                lo = max(0, hi - 64)
                for c in range(3):
                    v = np.zeros(64, np.float32)
                    v[:hi - lo] = g[a + lo:a + hi, c]
                    go[r, c] = _F(go[r, c] + _butterfly(v))
                    v = np.zeros(64, np.float32)
                    v[:hi - lo] = lg[a + lo:a + hi, c]
                    gdir[r, c] = _F(gdir[r, c] + _butterfly(v))
    return go, gdir
