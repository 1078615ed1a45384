"""The edge-case table of the fused march (tests/march_cases.py) restated for the march over a vector-matrix decomposed
density (csrc/march_vm.hip): test infrastructure, CPU only; used by tests/test_march_vm_host.py and
tests/test_gpu_march_vm.py.

A `march_cases.Scene` is a lattice X x 9 x 9 whose every line (j, k) along x carries its own density profile, so it is a
sum of products of an indicator of (j, k) and a profile along x, which is what the decomposition represents exactly:
    plane xy (rows y, columns z; its line runs along x): [1, R, 9, 9], line [1, R, X, 1]
      component 0       plane = AIR at every (j, k) whose dense line is all AIR and 0 elsewhere; line = 1
      component r >= 1  plane = 1 at one (j, k) with a line that is not all AIR and 0 elsewhere; line = density[:, j, k]
    planes and lines yz, zx: zeros of their natural sizes ([1, R, X, 9] / [1, R, 9, 1] and [1, R, 9, X] / [1, R, 9, 1]).
The bilinear plane value times the linear line value, summed over the components, is the trilinear value of the dense
grid; in float32 the two differ by the rounding of the products (measured on the CPU: at most 3.8e-6 on fine129, 0.0 on
fine1025 and coarse129), far inside the margin every row of the table keeps (march_cases.py, module text).
`pad`: R is padded with zero components to a multiple of 4, which the kernel's 16-byte loads need; unpadded R (26, 11, 3)
takes the element loads.

Left out, with the reason: `nan_scene` (the NaN of one voxel sits in a line of the decomposition, and NaN times a plane's 0
is NaN: the whole slab x = 40 is poisoned, not one voxel, so the row's statement is about another scene); the NDC scenes
(dvgo_march_vm_density refuses NDC spacing).
"""
import numpy as np

import march_cases as C
import march_oracle as M
import vm_density_oracle as DO

_F = np.float32
KEYS = DO.KEYS


def scenes():
    return [C.fine_scene(), C.long_scene(), C.coarse_scene()]


# what the issue's table states for these scenes: R padded / unpadded, rows, records
TABLE = {'fine129': (28, 26, 37, 2855), 'fine1025': (12, 11, 11, 8065), 'coarse129': (4, 3, 4, 874)}


def vm_tensors(sc, pad):
    """-> (planes, lines): dicts of float32 arrays [1, R, H, W] / [1, R, N, 1] restating `sc.density` (module text)."""
    X = sc.X
    air = np.all(sc.density == _F(C.AIR), axis=0)                   # [9, 9]: (j, k) whose line is all AIR
    own = [(j, k) for j in range(9) for k in range(9) if not air[j, k]]
    R = 1 + len(own)
    if pad:
        R = (R + 3) // 4 * 4
    planes = {'xy': np.zeros((1, R, 9, 9), _F), 'yz': np.zeros((1, R, X, 9), _F), 'zx': np.zeros((1, R, 9, X), _F)}
    lines = {'xy': np.zeros((1, R, X, 1), _F), 'yz': np.zeros((1, R, 9, 1), _F), 'zx': np.zeros((1, R, 9, 1), _F)}
    planes['xy'][0, 0][air] = C.AIR
    lines['xy'][0, 0, :, 0] = 1
    for r, (j, k) in enumerate(own, 1):
        planes['xy'][0, r, j, k] = 1
        lines['xy'][0, r, :, 0] = sc.density[:, j, k]
    return planes, lines


def cpu_forward_vm(sc, O, planes, lines):
    """`march_cases.cpu_forward` with the trilinear read replaced by the float64 oracle of the decomposed density rounded to
    float32: positions, occupancy, raw2alpha and alpha2weight are the C oracle's.  -> (Result, density [M] at the occupied
    samples, the dense trilinear density there)."""
    o, d = sc.arrays()
    N = o.shape[0]
    pts, out, ray_id, step_id, n_steps, t_min, _ = O.sample_pts_on_rays(o, d, sc.xyz_min, sc.xyz_max, sc.near, sc.far, float(_F(sc.stepdist)))
    pts, ray_id, step_id = pts[~out], ray_id[~out], step_id[~out]
    start = O.infer_ray_start_dir(o, d, t_min)[0]
    sel = O.maskcache_lookup(sc.mask, pts, sc.mask_scale, sc.mask_shift)
    pts, ray_id, step_id = pts[sel], ray_id[sel], step_id[sel]
    dens = DO.forward(planes, lines, pts, sc.xyz_min, sc.xyz_max)[0].astype(_F)
    dense = O.grid_sample_fwd(sc.density[None], pts, sc.xyz_min, sc.xyz_max, use_fma=True)[:, 0]
    with np.errstate(all='ignore'):
        exp_d, alpha = O.raw2alpha(dens, sc.act_shift, sc.interval)
    if sc.thres > 0:
        sel = alpha > _F(sc.thres)
        ray_id, step_id, exp_d, alpha = ray_id[sel], step_id[sel], exp_d[sel], alpha[sel]
    w, T, last, i_start, i_end = O.alpha2weight(alpha, ray_id, N)
    n2 = i_end - i_start
    rows = np.concatenate([np.arange(a, b) for a, b in zip(i_start, i_end)]).astype(np.int64)
    flag = (w[rows] > _F(sc.thres)) if sc.thres > 0 else np.ones(rows.shape[0], bool)
    s = (step_id[rows].astype(np.int64) | np.where(flag, 1 << 31, 0)).astype(np.uint32).view(np.int32)
    rec2 = np.stack([s.view(np.float32), exp_d[rows], alpha[rows], T[rows]], 1)
    R = M.Records(rec2, n2, np.concatenate([[0], np.cumsum(n2)])[:-1])
    return C.Result(R, np.bincount(R.ray, R.flag, N), last, n_steps, start), dens, dense


def rec_stride(sc):
    """fused._rec_stride for the scene: ceil((far - near) / stepdist) + 2"""
    return int(np.ceil((sc.far - sc.near) / sc.stepdist)) + 2
