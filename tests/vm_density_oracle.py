"""Oracle of the vector-matrix density (csrc/vm_density.hip; include/dvgo_hip.h, the VM density block), numpy, built on
tests/vm_oracle.py: the density is the row sum of the sampler's 3R products, and its gradient the sampler's gradient with
one float of incoming gradient per sample broadcast over the row.

forward  -> value [M] and A [M] = sum over the row of the products' magnitudes, float64.
backward -> vm_oracle.backward's ({key: (grad, A, n)}, {key: (grad, A, n)}) for grad_out [M].
sum32    -> the float32 sum of the float32 products in a given order ('ascending' or 'pairwise'): what a float32
            implementation may legitimately return, used to show that the forward bound holds for the reference alone.
"""
import numpy as np

import vm_oracle as VO

KEYS = VO.KEYS
U = VO.U
f32 = np.float32


def forward(planes, lines, xyz, mn, mx):
    val, A = VO.forward(planes, lines, xyz, mn, mx)
    return val.sum(1), A.sum(1)


def backward(planes, lines, xyz, mn, mx, grad_out):
    g = np.asarray(grad_out, np.float64).reshape(-1)
    R = np.asarray(planes[KEYS[0]]).shape[1]
    return VO.backward(planes, lines, xyz, mn, mx, np.broadcast_to(g[:, None], (g.shape[0], 3 * R)))


def forward_bound(R, A):
    """|got - ref| <= (3R + 12) U A: 12 U A_j per product (tests/test_gpu_vm.py), and 3R - 1 additions that each round a
    partial sum of magnitude at most A, in any order; rounded up by one."""
    return (3 * R + 12) * U * A


def sum32(planes, lines, xyz, mn, mx, order):
    """The 3R products rounded to float32 (from the float64 oracle values: one rounding each, inside their 12 U A_j), summed
    in float32 in the given order."""
    prod = VO.forward(planes, lines, xyz, mn, mx)[0].astype(f32)
    if order == 'ascending':
        acc = np.zeros(prod.shape[0], f32)
        for j in range(prod.shape[1]):
            acc = (acc + prod[:, j]).astype(f32)
        return acc
    assert order == 'pairwise'
    cols = [prod[:, j] for j in range(prod.shape[1])]
    while len(cols) > 1:
        nxt = [(cols[i] + cols[i + 1]).astype(f32) for i in range(0, len(cols) - 1, 2)]
        if len(cols) % 2:
            nxt.append(cols[-1])
        cols = nxt
    return cols[0]
