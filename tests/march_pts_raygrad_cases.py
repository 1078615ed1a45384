"""The cases of dvgo_march_ray_bwd_pts and dvgo_march_vm_ray_bwd (csrc/march_raygrad.hip) that the host tests
(tests/test_march_pts_raygrad_host.py: on the CPU oracle's records) and the GPU tests (tests/test_gpu_march_pts_raygrad.py: on
the device's) share: test infrastructure, CPU only, numpy.

  the edge-case tables   `march_cases.fine_scene` (dense) and `march_vm_cases` on fine129 / coarse129 (padded and unpadded R):
                         n2 in {0, 1, 63, 64, 65, 256}, stops on lane 63 and on lane 0 of the next chunk, flagged and unflagged
                         records in one ray.  The VM tables have zero yz / zx tensors: they test the walk.
  rand20                 a random 20^3 lattice over [-1, 1]^3 with 96 tilted rays from outside the box, density around the
                         activation's knee, an occupancy mask with holes, fast_color_thres = 1e-4 (flagged and unflagged
                         records); `vm20`: the same rays over six random non-zero tensors of 20 x 20 / 20, R components: the
                         derivative on every plane and line.
Seeds are chosen so that every ray of every case has a finite reference (the host test asserts it; no ray is left out).
`upstream` draws the gradients a launch is handed, the same on the host and on the device."""
import numpy as np

import march_cases as C

_F = np.float32
N_RAND = 96


def _rand_rays(sc, rng, n):
    for _ in range(n):
        a = rng.uniform(-0.8, 0.8, 3)
        dirn = rng.standard_normal(3)
        dirn /= np.linalg.norm(dirn)
        sc.ray(tuple(a - 2.5 * dirn), tuple(dirn * rng.uniform(0.5, 2.0)))


def _box20(name, rng):
    sc = C.Scene(name, 20, 1e-2, 1e-4, 0)
    sc.xyz_min, sc.xyz_max = np.full(3, -1.0, _F), np.full(3, 1.0, _F)
    sc.density = np.zeros((20, 20, 20), _F)
    sc.mask = rng.random((20, 20, 20)) < 0.9
    sc.stepdist = 0.5 * (2.0 / 19)
    sc.near, sc.far = 0.2, 6.0
    _rand_rays(sc, rng, N_RAND)
    return sc


def rand20_scene(seed=3):
    rng = np.random.default_rng(seed)
    sc = _box20('rand20', rng)
    sc.density = rng.normal(2.0, 4.0, sc.density.shape).astype(_F)
    return sc


def vm20_scene(R, seed=5):
    """-> (scene, planes, lines): six non-zero tensors [1,R,20,20] / [1,R,20,1]"""
    rng = np.random.default_rng(seed + R)
    sc = _box20(f'vm20-R{R}', rng)
    s = 1.6 / R ** 0.25                                  # the sum of 3R products keeps a spread of about 4.4
    planes = {k: (s * rng.standard_normal((1, R, 20, 20))).astype(_F) for k in ('xy', 'yz', 'zx')}
    lines = {k: (s * rng.standard_normal((1, R, 20, 1))).astype(_F) for k in ('xy', 'yz', 'zx')}
    return sc, planes, lines


def upstream(N, M3, seed):
    """-> grad_weights [M3], grad_last [N], grad_pts [M3,3] float32"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(M3).astype(_F), rng.standard_normal(N).astype(_F), rng.standard_normal((M3, 3)).astype(_F))
