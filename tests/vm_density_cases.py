"""Inputs and oracle results the vector-matrix density's host and GPU tests share: the shapes, the box and the `points()`
construction of tests/test_gpu_vm.py, by value, with one float of incoming gradient per sample."""
import functools

import numpy as np

import triplane_oracle as TO
import vm_density_oracle as DO
import vm_oracle as VO

SIZES = {'xy': (5, 7), 'yz': (6, 4), 'zx': (3, 9)}
LINES = {'xy': 6, 'yz': 1, 'zx': 9}
MS = (0, 1, 63, 64, 65, 1000)
RS = (1, 3, 4, 8)
MN, MX = np.array([-1.0, -0.8, -0.6], np.float32), np.array([0.9, 1.1, 0.7], np.float32)


def points(M, rng):
    """Random points up to 30 % of the box outside it; in front of them the eight box corners (both faces of every axis:
    exact lattice nodes, and on the upper face f + 1 is out of range), the lattice nodes of every plane and line, and
    points 0.8 box extents outside on each side: more than one cell of every axis here, so that all corners are out."""
    xyz = (MN + (MX - MN) * (rng.random((M, 3)) * 1.6 - 0.3)).astype(np.float32)
    special = [[(MN, MX)[(i >> a) & 1][a] for a in range(3)] for i in range(8)]
    for key, (H, W) in SIZES.items():
        ah, aw = TO.AXES[key]
        al, N = VO.LINE_AXIS[key], LINES[key]
        for i in range(4):
            p = (MN + (MX - MN) * rng.random(3)).astype(np.float32)
            p[ah] = MN[ah] + (MX[ah] - MN[ah]) * np.float32((i % H) / max(H - 1, 1))
            p[aw] = MN[aw] + (MX[aw] - MN[aw]) * np.float32((i % W) / max(W - 1, 1))
            p[al] = MN[al] + (MX[al] - MN[al]) * np.float32((i % N) / max(N - 1, 1))
            special.append(p)
    for side in (-0.8, 1.8):
        special.append(MN + (MX - MN) * np.float32(side))
        for a in range(3):
            p = (MN + (MX - MN) * np.float32(0.4)).astype(np.float32)
            p[a] = MN[a] + (MX[a] - MN[a]) * np.float32(side)
            special.append(p)
    special = np.array(special, np.float32)[:M]
    xyz[:len(special)] = special
    return xyz


def tensors(R, rng):
    planes = {k: rng.standard_normal((1, R, *hw)).astype(np.float32) for k, hw in SIZES.items()}
    lines = {k: rng.standard_normal((1, R, n, 1)).astype(np.float32) for k, n in LINES.items()}
    return planes, lines


@functools.lru_cache(maxsize=None)
def case(R):
    """Component count R -> planes, lines and, per M, (xyz, forward value and A, grad_out [M], backward reference)."""
    rng = np.random.default_rng(300 + R)
    planes, lines = tensors(R, rng)
    per_m = {}
    for M in MS:
        xyz = points(M, rng)
        val, A = DO.forward(planes, lines, xyz, MN, MX)
        gout = rng.standard_normal(M).astype(np.float32)
        per_m[M] = (xyz, val, A, gout, DO.backward(planes, lines, xyz, MN, MX, gout))
    return planes, lines, per_m


def dyadic_case(rng, M=300, R=4):
    """tests/test_gpu_vm.py's dyadic case: box [-1, 1]^3 and points on multiples of 2^-10 in [-1.25, 1.25], where every
    float32 coordinate operation of the kernel is exact."""
    mn, mx = np.float32([-1, -1, -1]), np.float32([1, 1, 1])
    xyz = (rng.integers(-1280, 1281, (M, 3)) / 1024.0).astype(np.float32)
    planes = {k: (0.5 * rng.standard_normal((1, R, *hw))).astype(np.float32) for k, hw in SIZES.items()}
    lines = {k: (0.5 * rng.standard_normal((1, R, n, 1))).astype(np.float32) for k, n in LINES.items()}
    gout = rng.standard_normal(M).astype(np.float32)
    return mn, mx, xyz, planes, lines, gout
