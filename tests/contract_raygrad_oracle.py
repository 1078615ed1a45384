"""float64 statement of the contraction's ray gradient (test infrastructure): what dvgo_contract_ray_bwd and
dvgo_contract_ray_bwd_rec (csrc/contract_raygrad.hip; include/dvgo_hip.h states the float32 arithmetic) must give.

The discontinuous choices are the kernel's: o', d', ||u|| and p = o' + d' * t are formed in float32 by the expressions of the
forward as tests/unbounded_oracle.py restates them (`sample`: the ray setup; `contract`: the norm and the inner flag), and the
inner flag and the inf-norm's arg-max axis (the LOWEST index attaining max|p_a|) are taken from those float32 values.  From
there on everything is float64: the contraction's Jacobian, the per-ray sums and the ray's own Jacobian.

  ray_setup(...)       o', d', ||u|| in float32
  points(...)          p [M,3] float32, inner [M], axis [M] of the listed samples
  ray_grads(...)       grad_o, grad_d [N,3] float64; abs_o, abs_d [N,3]: per ray and component the sum of the absolute values
                       of the terms the result is made of, with f and f' split into their two pieces each, so that the
                       cancellation of f' near n = 1 (bg_len = 1: f'(1) = 0) counts in full; n_ray [N]
  bound(...)           (n_ray + ROUNDINGS) * 2^-24 * abs: see ROUNDINGS
  restate_f32(...)     the kernel's arithmetic in float32 numpy (correctly rounded, no contraction), summed per ray in the
                       kernel's order ('lanes': 64 accumulators by position modulo 64, then the butterfly) or front to back
                       ('sequential')
"""
import numpy as np

import unbounded_oracle as U

f32 = np.float32

# Roundings on the longest chain from the float32 inputs (o', d', ||u||, p, t, g: exact inputs of both sides) to one term of
# grad_d, each at most 2^-24 relative to the absolute value of the term it is part of.  u = one rounding.
#   n ('l2'): three squares (1u each on positive addends), two adds (2u), halved by the square root, the root itself: 2.5u
#   w = p_a / n: 2.5 + 1                                                                                    =  3.5
#   f' = ((2b)/n - (1+b)) / (n*n): (2b)/n 3.5 | (1+b) 1 -> 3.5, the subtraction 1 (relative to the two pieces, which
#        abs_* counts separately), n*n 2 * 2.5 + 1, the division 1                                         = 11.5
#   p . g: a product and two adds                                                                          =  3
#   c = f' * (p . g), w * c, f g + w c                                                                     =  3
#   t * h                                                                                                  =  1
#   (the other term, f g with f = ((1+b) - b/n) / n, is shorter: 3.5 + 1 + 3.5 + 1 + 1)
#   the ray: d' . B a product and two adds 3, d' * (d' . B) 1, B - ... 1, / ||u|| 1, / r 1                 =  7
# 29 in all; 32 leaves room for the second-order terms ((1 + 2^-24)^k - 1 < 1.0001 k 2^-24 for k < 1000).  The sum of the n_ray
# terms of one ray adds at most n_ray - 1 roundings in any order, each relative to a partial sum that abs_* bounds.
ROUNDINGS = 32
EPS = 2.0 ** -24


def ray_setup(rays_o, rays_d, center, radius, dtype=f32):
    """-> o' [N,3], d' [N,3], ||u|| [N] in float32: the first lines of unbounded_oracle.sample.  (`dtype` float64: the same
    expressions on float64 inputs, for the comparison with autograd, where no float32 forward exists.)"""
    rays_o, rays_d = np.asarray(rays_o, dtype), np.asarray(rays_d, dtype)
    c, r = np.asarray(center, dtype), np.asarray(radius, dtype)
    o = (rays_o - c) / r
    u = rays_d / r
    nu = np.sqrt(u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1] + u[:, 2] * u[:, 2])
    return o, u / nu[:, None], nu


def points(o, d, t_tab, b, norm, ray_id, step_id, dtype=f32):
    """p of the listed samples, the forward's norm and inner flag, the arg-max axis (lowest index) and t: float32."""
    t = np.asarray(t_tab, dtype)[step_id]
    p = (o[ray_id] + d[ray_id] * t[:, None]).astype(dtype)
    if dtype is f32:
        _, n, inner = U.contract(p, b, norm)
    else:
        n = np.abs(p).max(-1) if norm == 'inf' else np.sqrt((p * p).sum(-1))
        inner = n <= 1
    axis = np.argmax(np.abs(p), axis=-1)            # numpy returns the first index of the maximum
    return p, n, inner, axis, t


def _jacobian_t(p, inner, axis, b, norm, g):
    """float64 h = J^T g per sample and the sum of absolute terms |h|_abs."""
    p64, g64 = p.astype(np.float64), np.asarray(g, np.float64)
    b = float(f32(b))                               # what the kernel is handed
    M = p.shape[0]
    if norm == 'inf':
        n = np.abs(p64[np.arange(M), axis])
        w = np.zeros_like(p64)
        w[np.arange(M), axis] = np.sign(p64[np.arange(M), axis])
    else:
        n = np.sqrt((p64 * p64).sum(-1))
        with np.errstate(divide='ignore', invalid='ignore'):
            w = p64 / n[:, None]
    with np.errstate(divide='ignore', invalid='ignore'):
        f = (1 + b) / n - b / n ** 2
        fp = -(1 + b) / n ** 2 + 2 * b / n ** 3
        f_abs = (1 + b) / n + b / n ** 2
        fp_abs = (1 + b) / n ** 2 + 2 * b / n ** 3
        dot = (p64 * g64).sum(-1)
        dot_abs = np.abs(p64 * g64).sum(-1)
        h = f[:, None] * g64 + w * (fp * dot)[:, None]
        h_abs = f_abs[:, None] * np.abs(g64) + np.abs(w) * (fp_abs * dot_abs)[:, None]
    h = np.where(inner[:, None], g64, h)
    h_abs = np.where(inner[:, None], np.abs(g64), h_abs)
    return h, h_abs


def ray_grads(rays_o, rays_d, center, radius, t_tab, b, norm, g, ray_id, step_id, dtype=f32):
    """-> dict grad_o, grad_d, abs_o, abs_d [N,3] float64 and n_ray [N].  `dtype`: the forward's (see ray_setup)."""
    N = np.asarray(rays_o).shape[0]
    ray_id, step_id = np.asarray(ray_id, np.int64), np.asarray(step_id, np.int64)
    o, d, nu = ray_setup(rays_o, rays_d, center, radius, dtype)
    p, _, inner, axis, t = points(o, d, t_tab, b, norm, ray_id, step_id, dtype)
    h, h_abs = _jacobian_t(p, inner, axis, b, norm, g)
    t64 = t.astype(np.float64)[:, None]
    A, B, Aa, Ba = (np.zeros((N, 3)) for _ in range(4))
    np.add.at(A, ray_id, h)
    np.add.at(B, ray_id, t64 * h)
    np.add.at(Aa, ray_id, h_abs)
    np.add.at(Ba, ray_id, t64 * h_abs)
    r64 = np.asarray(radius, dtype).astype(np.float64)
    d64, nu64 = d.astype(np.float64), nu.astype(np.float64)[:, None]
    dB = (d64 * B).sum(-1, keepdims=True)
    dB_abs = (np.abs(d64) * Ba).sum(-1, keepdims=True)
    return dict(grad_o=A / r64, grad_d=(B - d64 * dB) / nu64 / r64, abs_o=Aa / np.abs(r64),
                abs_d=(Ba + np.abs(d64) * dB_abs) / nu64 / np.abs(r64), n_ray=np.bincount(ray_id, minlength=N))


def bound(abs_terms, n_ray):
    return (np.asarray(n_ray, np.float64)[:, None] + ROUNDINGS) * EPS * abs_terms


def restate_f32(rays_o, rays_d, center, radius, t_tab, b, norm, g, ray_id, step_id, order='lanes'):
    """The kernel's float32 arithmetic, operation for operation (include/dvgo_hip.h) -> grad_o, grad_d [N,3] float32."""
    N = np.asarray(rays_o).shape[0]
    ray_id, step_id = np.asarray(ray_id, np.int64), np.asarray(step_id, np.int64)
    r = np.asarray(radius, f32)
    o, d, nu = ray_setup(rays_o, rays_d, center, radius)
    p, n, inner, axis, t = points(o, d, t_tab, b, norm, ray_id, step_id)
    g = np.asarray(g, f32)
    b = f32(b)
    one_b = f32(1) + b
    M = p.shape[0]
    with np.errstate(divide='ignore', invalid='ignore'):
        f = (one_b - b / n) / n
        fp = ((f32(2) * b) / n - one_b) / (n * n)
        c = fp * ((p[:, 0] * g[:, 0] + p[:, 1] * g[:, 1]) + p[:, 2] * g[:, 2])
        h = f[:, None] * g
        if norm == 'l2':
            h = h + (p / n[:, None]) * c[:, None]
        else:
            pa = p[np.arange(M), axis]
            h[np.arange(M), axis] = h[np.arange(M), axis] + np.where(pa < 0, -c, c)
    h = np.where(inner[:, None], g, h).astype(f32)
    th = (t[:, None] * h).astype(f32)
    off = np.searchsorted(ray_id, np.arange(N + 1))
    out_o, out_d = np.zeros((N, 3), f32), np.zeros((N, 3), f32)
    for ray in range(N):
        a, e = off[ray], off[ray + 1]
        if a == e:
            continue
        AB = np.concatenate([h[a:e], th[a:e]], -1)              # [n,6]
        if order == 'lanes':
            acc = np.zeros((64, 6), f32)
            for base in range(0, e - a, 64):
                chunk = AB[base:base + 64]
                acc[:chunk.shape[0]] = acc[:chunk.shape[0]] + chunk
            for s in (32, 16, 8, 4, 2, 1):                      # v += shfl_xor(v, s)
                acc = acc + acc[np.arange(64) ^ s]
            tot = acc[0]
        else:
            tot = np.zeros(6, f32)
            for row in AB:
                tot = tot + row
        A, B = tot[:3], tot[3:]
        dB = (d[ray, 0] * B[0] + d[ray, 1] * B[1]) + d[ray, 2] * B[2]
        out_o[ray] = A / r
        out_d[ray] = ((B - d[ray] * dB) / nu[ray]) / r
    return out_o, out_d
