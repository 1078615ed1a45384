"""Distortion loss of unbounded scenes, host side of csrc/contract.hip (dvgo_distortion_fwd_bwd).

The Mip-NeRF 360 regulariser (Barron et al., "Mip-NeRF 360: Unbounded Anti-Aliased Neural Radiance Fields", CVPR 2022)
in the O(n) per-ray form used by DVGO v2 (Sun et al., arXiv:2206.05085).  For the kept samples of each ray in step
order, with s the normalised distance of each sample and delta = 1 / n_max:

    L = (1/N) sum_rays [ 2 sum_i w_i (s_i W_<i - S_<i) + (1/3) delta sum_i w_i^2 ]
    W_<i = sum_{j<i} w_j,   S_<i = sum_{j<i} w_j s_j

which equals (1/N) sum_rays [ sum_ij w_i w_j |s_i - s_j| + (1/3) delta sum_i w_i^2 ] when s increases along the ray.
One launch computes the value and dL/dw; both are bitwise repeatable (fixed-order reductions, no float atomics).
"""
import torch

from . import _lib as L
from ._lib import _i64, _int, check_f32, check_input, ptr, stream_of

_BLOCK = 256          # DVGO_DIST_BLOCK of csrc/contract.hip


class DistortionLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weights, s, n_max, ray_id, n_rays):
        w = weights.contiguous()
        s = s.contiguous()
        check_input(w, 'weights'); check_f32(w, 'weights')
        check_input(s, 's'); check_f32(s, 's')
        check_input(ray_id, 'ray_id')
        if ray_id.dtype != torch.int64:
            raise RuntimeError('ray_id must be int64')
        if not (w.dim() == 1 and w.shape == s.shape == ray_id.shape):
            raise RuntimeError('weights, s and ray_id must be 1-D of one length')
        n_rays, n_max = int(n_rays), int(n_max)
        if n_rays <= 0 or n_max <= 0:
            raise ValueError('distortion_loss needs n_rays > 0 and n_max > 0')
        M = w.shape[0]
        dev = w.device
        grad = torch.empty_like(w)
        nb = (n_rays + _BLOCK - 1) // _BLOCK
        ws = torch.zeros(1 + nb, dtype=torch.float64, device=dev)      # [0]: the ticket (uint32 in the low word), then partials
        loss = torch.empty((), dtype=torch.float32, device=dev)
        with L.device_of(w):
            L.call('dvgo_distortion_fwd_bwd', ptr(w), ptr(s), ptr(ray_id), _i64(M), _i64(n_rays), _i64(n_rays), _int(n_max),
                   ptr(grad), L._vp(ws.data_ptr() + 8), ptr(ws), ptr(loss), stream_of(w))
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, go):
        (grad,) = ctx.saved_tensors
        return grad * go, None, None, None, None


def distortion_loss(weights, s, n_max, ray_id, n_rays):
    """Distortion loss of the kept samples (`weights`, `s` [M] grouped by the sorted `ray_id` in step order), normalised
    by `n_rays`.  Differentiable w.r.t. `weights` only."""
    return DistortionLoss.apply(weights, s, n_max, ray_id, n_rays)
