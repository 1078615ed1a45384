"""The whole contracted render as a differentiable function of its RAYS, in plain torch ops of any float dtype on the CPU
(test infrastructure): what a user would write without the kernels.  The set of kept samples is an input and fixed, as the
contract of DirectContractedVoxGO(raygrad=True) has it; everything else is restated from the module docstring of
directvoxgo_amd/dcvgo.py: contraction -> F.grid_sample (trilinear, align_corners=True, zero padding) of the density ->
alpha = 1 - (1 + exp(raw + act_shift))^-interval -> transmittance and weights over the kept samples -> sigmoid(k0) colours
(rgbnet_dim = 0) -> composite with the background, and the distortion loss in its O(n^2) definition with s = 1 - 1 / (1 + t).

tests/test_gpu_contract_raygrad.py runs it in float64 (the reference of the end-to-end test) and in float32 (that test's
yardstick: the error any float32 evaluation of this chain has).
"""
import torch
import torch.nn.functional as F


def contract(rays_o, rays_d, center, radius, t_tab, b, norm):
    """-> q [N,K,3]: the contracted sample of every ray at every distance of the table."""
    o = (rays_o - center) / radius
    u = rays_d / radius
    d = u / u.norm(dim=-1, keepdim=True)
    p = o[:, None, :] + d[:, None, :] * t_tab[None, :, None]
    n = p.abs().amax(-1) if norm == 'inf' else p.norm(dim=-1)
    f = (1 + b) / n - b / n ** 2
    return torch.where((n <= 1)[..., None], p, p * f[..., None])


def _sample(grid, q, lim):
    """grid [C,X,Y,Z], q [M,3] in [-lim, lim]^3 -> [M,C] (the model's grid_sampler)."""
    g = ((q + lim) / (2 * lim)).flip(-1) * 2 - 1
    out = F.grid_sample(grid[None], g[None, None, None], mode='bilinear', align_corners=True)
    return out[0, :, 0, 0].t()


def render(rays_o, rays_d, ray_id, step_id, t_tab, center, radius, b, norm, density, k0, act_shift, interval, bg,
           stop_after=None):
    """rays_o, rays_d [N,3] (leaves of the dtype everything else is given in); ray_id, step_id [M] int64: the kept samples,
    ray-major and step-ascending.  density [X,Y,Z], k0 [3,X,Y,Z].  -> dict rgb_marched [N,3], weights [M], alphainv_last [N].
    `stop_after` [M] bool, optional: samples behind their ray's early stop (they carry weight 0 and do not enter the
    transmittance; the fused march's kept set contains none)."""
    N, K = rays_o.shape[0], t_tab.shape[0]
    q = contract(rays_o, rays_d, center, radius, t_tab, b, norm)[ray_id, step_id]
    lim = 1 + b
    alpha = 1 - (1 + torch.exp(_sample(density[None], q, lim)[:, 0] + act_shift)) ** (-interval)
    through = 1 - alpha + 1e-10
    if stop_after is not None:
        alpha = torch.where(stop_after, torch.zeros_like(alpha), alpha)
        through = torch.where(stop_after, torch.ones_like(through), through)
    Ta = torch.cumprod(torch.ones((N, K), dtype=rays_o.dtype).index_put((ray_id, step_id), through), 1)
    Tb = torch.cat([torch.ones((N, 1), dtype=rays_o.dtype), Ta[:, :-1]], 1)
    weights = Tb[ray_id, step_id] * alpha
    last = Ta[:, -1]
    rgb = torch.sigmoid(_sample(k0, q, lim))
    marched = torch.zeros((N, 3), dtype=rays_o.dtype).index_add(0, ray_id, weights[:, None] * rgb) + last[:, None] * bg
    return dict(rgb_marched=marched, weights=weights, alphainv_last=last)


def distortion(weights, ray_id, step_id, t_tab, n_rays):
    """The distortion loss of distortion.py by its definition: (1/N) sum_rays [sum_ij w_i w_j |s_i - s_j| + sum_i w_i^2 / (3 n_max)],
    s = 1 - 1 / (1 + t) a constant."""
    K = t_tab.shape[0]
    s = 1 - 1 / (1 + t_tab)
    W = torch.zeros((n_rays, K), dtype=weights.dtype).index_put((ray_id, step_id), weights)
    pair = (W[:, :, None] * W[:, None, :] * (s[:, None] - s[None, :]).abs()[None]).sum()
    return (pair + (W * W).sum() / (3 * K)) / n_rays
