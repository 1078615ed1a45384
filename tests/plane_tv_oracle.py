"""numpy statement of dvgo_plane_reg_add_grad (include/dvgo_hip.h): the total-variation and L1
gradient of a plane-shaped parameter added to its gradient, in two forms.

  reg32   float32, one rounding per operation in the stated order (w-, w+, h-, h+, L1, then grad + g): the BIT reference.
  reg64   the same in float64 on the same float32 inputs and float32 weights: the VALUE reference, with the magnitude
          A = |g0| + sum |w * clamp| + |wl1| the error bound of tests/test_plane_tv_host.py is stated in.

Arrays are [C, H, W]; a line is [R, N, 1].  Also the inputs the GPU test and the host test share (`tensor`, `six`,
`weights_of`): parameters 1.5 * randn so that the clamp is active on part of the differences, with planted pairs of exactly
equal neighbours and exact zeros (one of them -0.0) for sgn; gradients with about half of their elements exactly zero, some of
those -0.0.
"""
import numpy as np

U = 2.0 ** -24
KEYS = ('xy', 'yz', 'zx')
SIZES = {'xy': (5, 7), 'yz': (6, 4), 'zx': (3, 9)}          # the shapes of tests/test_gpu_vm.py
LINES = {'xy': 6, 'yz': 1, 'zx': 9}


def _terms(p, wh, ww, wl1, f):
    """[(slice of the elements that have the term, the term there)] in the stated order, every operation in dtype f."""
    one = f(1)
    c1 = lambda v: np.minimum(np.maximum(v, -one), one)                       # noqa: E731
    out = []
    W, H = p.shape[2], p.shape[1]
    if W > 1:
        out.append((np.s_[:, :, 1:], ww * c1(p[:, :, 1:] - p[:, :, :-1])))
        out.append((np.s_[:, :, :-1], ww * c1(p[:, :, :-1] - p[:, :, 1:])))
    if H > 1:
        out.append((np.s_[:, 1:, :], wh * c1(p[:, 1:, :] - p[:, :-1, :])))
        out.append((np.s_[:, :-1, :], wh * c1(p[:, :-1, :] - p[:, 1:, :])))
    if wl1 != 0:
        sgn = (p > 0).astype(f) - (p < 0).astype(f)                           # sgn(+-0) = +0
        out.append((np.s_[:, :, :], wl1 * sgn))
    return out


def reg32(param, grad, wh, ww, wl1, dense_mode):
    """-> the new gradient, float32 [C,H,W], bit for bit what the kernel must leave."""
    f = np.float32
    p, g0 = np.asarray(param, f), np.asarray(grad, f)
    assert p.ndim == 3 and p.shape == g0.shape
    g = np.zeros_like(p)
    for sl, t in _terms(p, f(wh), f(ww), f(wl1), f):
        assert t.dtype == f
        g[sl] = g[sl] + t
    out = g0 + g
    if not dense_mode:
        skip = g0 == 0                                                        # +0.0 and -0.0: left untouched, bits included
        out[skip] = g0[skip]
    assert out.dtype == f
    return out


def reg64(param, grad, wh, ww, wl1, dense_mode):
    """-> (the new gradient, A), float64 [C,H,W]; the weights are the float32 values the kernel receives."""
    d = np.float64
    p, g0 = np.asarray(param, np.float32).astype(d), np.asarray(grad, np.float32).astype(d)
    wh, ww, wl1 = (d(np.float32(w)) for w in (wh, ww, wl1))
    g, A = np.zeros_like(p), np.abs(g0)
    for sl, t in _terms(p, wh, ww, wl1, d):
        g[sl] += t
        A[sl] += np.abs(t)
    if wl1 != 0:
        A += abs(wl1) * (p == 0)                                              # the L1 term counts as |wl1| everywhere
    out = g0 + g
    if not dense_mode:
        skip = g0 == 0
        out[skip], A[skip] = g0[skip], 0.0
    return out, A


# ---------------------------------------------------------------------------------------------- shared inputs
def tensor(rng, C, H, W):
    """(param, grad) float32 [C,H,W] with the planted values described in the module docstring."""
    p = (1.5 * rng.standard_normal((C, H, W))).astype(np.float32)
    n = p.size
    flat = p.reshape(-1)                                                      # (a view: [C,H,W] is contiguous)
    zeros = rng.choice(n, size=min(n, max(1, n // 16)), replace=False)
    flat[zeros] = 0.0
    if n > 1:
        flat[zeros[0]] = -0.0
    for _ in range(max(4, n // 12) if max(H, W) > 1 else 0):                  # pairs of exactly equal neighbours
        c, h, w = (int(rng.integers(0, s)) for s in (C, H, W))
        along_w = W > 1 and (H == 1 or rng.random() < 0.5)
        h, w = (h, max(w, 1)) if along_w else (max(h, 1), w)
        if p[c, h, w] != 0:                                                   # (the planted zeros stay)
            p[c, h, w] = p[c, h, w - 1] if along_w else p[c, h - 1, w]
    g = rng.standard_normal((C, H, W)).astype(np.float32)
    u = rng.random((C, H, W))
    g[u < 0.5] = 0.0
    g[u < 0.15] = -0.0
    return p, g


def six(R, seed):
    """The six tensors of a VM model with the shapes above: three planes [R,H,W], then three lines [R,N,1]."""
    rng = np.random.default_rng(seed)
    return [tensor(rng, R, *SIZES[k]) for k in KEYS] + [tensor(rng, R, LINES[k], 1) for k in KEYS]


def weights_of(n, l1):
    """n distinct (wh, ww, wl1) triples; wl1 alternates in sign when `l1`, else 0."""
    return [(0.3 + 0.11 * k, 0.9 - 0.07 * k, ((-1) ** k) * 0.013 * (k + 1) if l1 else 0.0) for k in range(n)]


def big(seed, R=16):
    """A plane whose channels-last row (130 * 16 = 2080 floats) makes a workgroup's threads loop over it, then a small
    plane and a line so that the block table crosses tensors."""
    rng = np.random.default_rng(seed)
    return [tensor(rng, R, 70, 130), tensor(rng, R, 3, 9), tensor(rng, R, 9, 1)]
