"""DirectContractedVoxGO: a voxel grid over a contracted space, for unbounded (360-degree, real-background) scenes.

Formulas from DVGO v2 (Sun et al., "Improved Direct Voxel Grid Optimization for Radiance Fields Reconstruction",
arXiv:2206.05085), which borrows the scene contraction and the distortion loss of Mip-NeRF 360 (Barron et al., CVPR
2022).  The reference code base has no such model; the contract is the sampler stated in `contracted_sample` and
restated in float32 by tests/unbounded_oracle.py, which the HIP sampler matches bit for bit.

Geometry.  `xyz_min` / `xyz_max` are the FOREGROUND box.  Per axis, c = (min + max) / 2 and r = (max - min) / 2 map it
to [-1, 1]^3; everything beyond is contracted into the shell 1 < |q| <= 1 + b (b = `bg_len`, norm `contracted_norm`:
'inf' for the max norm, 'l2').  The grids live on a cubic W^3 lattice over [-(1+b), 1+b]^3 (the `xyz_min` / `xyz_max`
buffers hold these contracted bounds; `get_kwargs` returns the foreground box).

Forward, in the order of DirectVoxGO.forward: contracted sampling with the occupancy lookup (csrc/contract.hip) ->
density trilinear -> Raw2Alpha -> alpha filter -> Alphas2Weights -> weight filter -> k0 trilinear and colour (the HIP
colour head where its shapes allow) -> composite with render_kwargs['bg'].  `near` and `far` are accepted and ignored:
the sample distances are a fixed table (`contracted_t_table`) in normalised units, from the ray origin to infinity.
The result carries, besides DirectVoxGO's keys, `step_id`, `t`, `s = 1 - 1/(1+t)` (per kept sample) and `n_max`;
`depth` (render_depth) is sum_i w_i t_i in normalised units (the foreground box has half-size 1 on every axis).
NDC rays, posbase_pe, voxel_count_views / maskout_near_cam_vox and mesh extraction are not supported.

`fused_march=True` (constructor option, default False; a plain attribute like DirectVoxGO.fused_raygrad: `get_kwargs` keeps
the key set its checkpoints have always had, so pass it to the constructor or to `load_model(..., fused_march=True)`):
`forward` runs fused.fused_march_contract (csrc/march_contract.hip: sampler, thinning, occupancy, density, alpha, both
filters and the transmittance in one launch, one wavefront per ray, nothing evaluated behind a ray's stop) -> k0 trilinear
at the kept positions -> colour -> the same composite.  Same result keys, same expressions for `s` and `depth`, and the
same bits as the op-by-op path in every key, with one documented exception shared with DirectVoxGO's fused march: with
fast_color_thres == 0 the op-by-op path also lists the samples behind a ray's stop, with weight exactly 0, which the march
never visits.  When the march's fixed-stride records would exceed fused._MAX_STRIDE_SCRATCH_BYTES the forward goes op by op.
Rays that require grad are refused, unless `raygrad=True`.  INTEGRATION.md section 5b is the contract.

`raygrad=True` (constructor option, default False; a plain attribute like `fused_march`, not a `get_kwargs` key and not in
checkpoints: pass it to the constructor or to `load_model(..., raygrad=True)`): with grad mode on and `rays_o` or `rays_d`
requiring grad, `forward` differentiates the render with respect to the rays, on either path (`_render` states the
stop-gradients and the tie rule).  The sample positions are wrapped in ops.contract_points, whose backward is
csrc/contract_raygrad.hip; on the fused march the density's share comes from the march's own backward
(fused.fused_march_contract(..., raygrad=True)).  Every result key keeps the bits of the forward without the option, and
with rays that do not require grad nothing changes.  pose.refine_poses accepts the model only with this option;
INTEGRATION.md section 7 is the contract.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from ._lib import _flt, _i64, _int, check_f32, check_input, ptr, stream_of
from .fused import ContractMarchConfig, composite, fused_march_contract
from .ops import contract_points, ray_offsets
from .voxel_model import VoxelModel, _as_f32, _check_rays, _rays_want_grad


def contracted_t_table(world, stepsize, bg_len):
    """-> (t float32 [n_max], N_in, n_max): N_in midpoints of a uniform split of [0, 2] and N_in of a split of [2, 256]
    uniform in 1/t; built in float64, rounded once to float32."""
    n_in = int(np.floor(2 / (2 + 2 * bg_len) * world / stepsize)) + 1
    b_in = np.linspace(0, 2, n_in + 1)
    b_out = 2 / np.linspace(1, 1 / 128, n_in + 1)
    mid = lambda b: (b[1:] + b[:-1]) / 2       # noqa: E731
    t = np.concatenate([mid(b_in), mid(b_out)]).astype(np.float32)
    return t, n_in, 2 * n_in


def thinning_threshold(world, stepsize, bg_len):
    """Contracted-space distance between two kept samples outside the unit box: 0.95 of a step of the lattice."""
    return float(np.float32((2 + 2 * bg_len) / world * stepsize * 0.95))


def contracted_sample(rays_o, rays_d, center, radius, t_tab, bg_len, contracted_norm, thres, mask_cache=None):
    """The contracted sampler (csrc/contract.hip), per ray in float32:

        o' = (o - c) / r;  u = d / r;  d' = u / ||u||_2;  p_k = o' + d' * t_k  (k < n_max = len(t_tab))
        n_k = max|p_k| ('inf') or ||p_k||_2 ('l2');  q_k = p_k if n_k <= 1 else p_k / n_k * ((1 + b) - b / n_k)
        kept: (n_k <= 1 or over_k) and mask_cache(q_k);  over_0 = False,
              k >= 1: acc += ||q_k - q_{k-1}||_2;  over_k = acc > thres;  acc = 0 when over_k

    -> (q [M,3], ray_id [M], step_id [M] int64, t [M]) of the kept samples, ray-major and step-ascending.  One host
    synchronisation (the total count).  rays_d must have no zero-length row."""
    check_input(rays_o, 'rays_o'); check_f32(rays_o, 'rays_o')
    check_input(rays_d, 'rays_d'); check_f32(rays_d, 'rays_d')
    for x, n in ((center, 'center'), (radius, 'radius'), (t_tab, 't_tab')):
        check_input(x, n); check_f32(x, n)
    if contracted_norm not in ('inf', 'l2'):
        raise ValueError(f"contracted_norm must be 'inf' or 'l2', got {contracted_norm!r}")
    N, n_max, dev = rays_o.shape[0], t_tab.shape[0], rays_o.device
    l2 = _int(1 if contracted_norm == 'l2' else 0)
    if mask_cache is not None:
        mask = mask_cache.mask.contiguous()
        if mask.dtype != torch.bool:
            raise RuntimeError('mask must be bool')
        mi, mj, mk = (int(v) for v in mask.shape)
        mext = (ptr(mask), _int(mi), _int(mj), _int(mk), ptr(mask_cache.xyz2ijk_scale.contiguous()),
                ptr(mask_cache.xyz2ijk_shift.contiguous()))
    else:
        mext = (ptr(None), _int(0), _int(0), _int(0), ptr(None), ptr(None))
    head = (ptr(rays_o), ptr(rays_d), _i64(N), ptr(center), ptr(radius), ptr(t_tab), _int(n_max), _flt(float(bg_len)), l2,
            _flt(float(thres))) + mext
    counts = torch.empty(N, dtype=torch.int32, device=dev)
    offsets = torch.empty(N + 1, dtype=torch.int64, device=dev)
    with L.device_of(rays_o):
        st = stream_of(rays_o)
        L.call('dvgo_contract_count', *head, ptr(counts), st)
        L.call('dvgo_exclusive_scan_i32', ptr(counts), _i64(N), ptr(offsets), st)
        M = int(offsets[N])                                                  # the one host synchronisation
        q = torch.empty((M, 3), dtype=torch.float32, device=dev)
        ray_id = torch.empty(M, dtype=torch.int64, device=dev)
        step_id = torch.empty(M, dtype=torch.int64, device=dev)
        t = torch.empty(M, dtype=torch.float32, device=dev)
        if M:
            L.call('dvgo_contract_emit', *head, ptr(offsets), ptr(q), ptr(ray_id), ptr(step_id), ptr(t), st)
    return q, ray_id, step_id, t


class DirectContractedVoxGO(VoxelModel):
    """Voxel grids over the contracted space of an unbounded scene (see the module docstring)."""

    def __init__(self, xyz_min, xyz_max, num_voxels=0, num_voxels_base=0, alpha_init=None,
                 mask_cache_world_size=None, fast_color_thres=0, bg_len=0.2, contracted_norm='inf',
                 rgbnet_dim=0, rgbnet_direct=True, rgbnet_depth=3, rgbnet_width=128, viewbase_pe=4, fused=True,
                 posbase_pe=0, fused_march=False, raygrad=False):
        super().__init__()
        if posbase_pe:
            raise NotImplementedError('posbase_pe is not supported by DirectContractedVoxGO')
        if contracted_norm not in ('inf', 'l2'):
            raise ValueError(f"contracted_norm must be 'inf' or 'l2', got {contracted_norm!r}")
        self.fused = bool(fused)
        self.fused_march = bool(fused_march)      # forward on fused.fused_march_contract; not in get_kwargs (module docstring)
        self.raygrad = bool(raygrad)              # rays that require grad are differentiated; not in get_kwargs (module docstring)
        self.fused_shade = True
        self.channels_last = True
        self.posbase_pe = 0
        fg_min, fg_max = _as_f32(xyz_min), _as_f32(xyz_max)
        self._fg_min_cpu, self._fg_max_cpu = fg_min.clone(), fg_max.clone()
        self.register_buffer('scene_center', (fg_min + fg_max) * 0.5)
        self.register_buffer('scene_radius', (fg_max - fg_min) * 0.5)
        self.bg_len = float(bg_len)
        self.contracted_norm = contracted_norm
        lim = 1 + self.bg_len
        self._set_box(torch.full((3,), -lim, dtype=torch.float32), torch.full((3,), lim, dtype=torch.float32))
        self.fast_color_thres = fast_color_thres

        self.num_voxels_base = num_voxels_base
        self.voxel_size_base = ((self._xyz_max_cpu - self._xyz_min_cpu).prod() / self.num_voxels_base).pow(1 / 3)
        self.alpha_init = alpha_init
        self.act_shift = np.log(1 / (1 - alpha_init) - 1)
        self._set_grid_resolution(num_voxels)

        ws = [int(v) for v in self.world_size]
        self.density = nn.Parameter(torch.zeros([1, 1, *ws]))
        self.rgbnet_kwargs = {'rgbnet_dim': rgbnet_dim, 'rgbnet_direct': rgbnet_direct, 'rgbnet_depth': rgbnet_depth,
                              'rgbnet_width': rgbnet_width, 'viewbase_pe': viewbase_pe}
        if rgbnet_dim > 0:
            self.rgbnet_direct = rgbnet_direct
        self._init_colour(ws, rgbnet_dim, rgbnet_dim if rgbnet_direct else rgbnet_dim - 3, viewbase_pe, rgbnet_width,
                          rgbnet_depth)

        self.mask_cache_world_size = None if mask_cache_world_size is None else [int(v) for v in mask_cache_world_size]
        self._set_mask_cache(torch.ones(self.mask_cache_world_size or ws, dtype=torch.bool))
        self._tab_cache = {}

    def _set_grid_resolution(self, num_voxels):
        """DirectVoxGO._set_grid_resolution on the contracted cube: the lattice is W^3."""
        self.num_voxels = num_voxels
        ext = self._xyz_max_cpu - self._xyz_min_cpu
        self.voxel_size = (ext.prod() / num_voxels).pow(1 / 3)
        self.world_size = (ext / self.voxel_size).long()
        self.voxel_size_ratio = self.voxel_size / self.voxel_size_base
        self._tab_cache = {}

    @property
    def world(self):
        return int(self.world_size[0])

    def get_kwargs(self):
        return {
            'xyz_min': self._fg_min_cpu.numpy(), 'xyz_max': self._fg_max_cpu.numpy(),
            'num_voxels': self.num_voxels, 'num_voxels_base': self.num_voxels_base,
            'alpha_init': self.alpha_init, 'act_shift': self.act_shift, 'voxel_size_ratio': self.voxel_size_ratio,
            'mask_cache_world_size': self.mask_cache_world_size, 'fast_color_thres': self.fast_color_thres,
            'bg_len': self.bg_len, 'contracted_norm': self.contracted_norm,
            **self.rgbnet_kwargs,
        }

    @torch.no_grad()
    def scale_volume_grid(self, num_voxels):
        """Trilinear resize of both grids to the new cubic lattice; the occupancy mask is rebuilt from the max-pooled
        activated density (at mask_cache_world_size when that is set)."""
        self._set_grid_resolution(num_voxels)
        ws = self._resize_grids()
        self_alpha = self._pooled_alpha()
        if self.mask_cache_world_size is not None and list(self.mask_cache_world_size) != list(ws):
            self_alpha = F.interpolate(self_alpha, size=tuple(self.mask_cache_world_size), mode='trilinear',
                                       align_corners=True)
        self._set_mask_cache(self_alpha[0, 0] > self.fast_color_thres)

    def maskout_near_cam_vox(self, cam_o, near):
        raise NotImplementedError('maskout_near_cam_vox is not built for contracted space')

    def voxel_count_views(self, *args, **kwargs):
        raise NotImplementedError('voxel_count_views (pervoxel_lr) is not built for contracted space')

    def _table(self, stepsize, device):
        key = (float(stepsize), str(device))
        tab = self._tab_cache.get(key)
        if tab is None:
            t, _, n_max = contracted_t_table(self.world, stepsize, self.bg_len)
            tab = (torch.from_numpy(t).to(device), n_max, thinning_threshold(self.world, stepsize, self.bg_len))
            self._tab_cache[key] = tab
        return tab

    def sample_ray(self, rays_o, rays_d, stepsize, **render_kwargs):
        """-> (q [M,3] contracted points, ray_id, step_id, t, n_max) of the kept samples (occupancy applied)."""
        t_tab, n_max, thres = self._table(stepsize, rays_o.device)
        q, ray_id, step_id, t = contracted_sample(rays_o.contiguous(), rays_d.contiguous(), self.scene_center,
                                                  self.scene_radius, t_tab, self.bg_len, self.contracted_norm, thres,
                                                  self.mask_cache)
        return q, ray_id, step_id, t, n_max

    def _march_contract_cfg(self, stepsize, device):
        """The fused march's constants for this step size, cached until the grids, the mask or the device change."""
        def make():
            t_tab, _, thres = self._table(stepsize, device)
            return ContractMarchConfig(
                self.scene_center, self.scene_radius, t_tab, self.bg_len, self.contracted_norm, thres, self.xyz_min,
                self.xyz_max, self.act_shift, float(stepsize * self.voxel_size_ratio), self.fast_color_thres,
                **self._mask_args())
        return self._cached_cfg((float(stepsize), str(device)), make)

    def forward(self, rays_o, rays_d, viewdirs, global_step=None, **render_kwargs):
        """Volume rendering in contracted space; see the module docstring for the order and the extra keys.
        `near` / `far` in render_kwargs are ignored; `ndc` rays are not supported.  With grad mode on, rays that require
        grad and `raygrad=True` the sample positions are wrapped in ops.contract_points (`_render` states what that means)."""
        _check_rays(rays_o)
        stepsize, wrap = render_kwargs['stepsize'], None
        if _rays_want_grad(rays_o, rays_d):
            if self.raygrad:
                rays_o, rays_d, viewdirs = rays_o.contiguous(), rays_d.contiguous(), viewdirs.detach()
                t_tab = self._table(stepsize, rays_o.device)[0]
                wrap = lambda q, ray_id, step_id: contract_points(      # noqa: E731
                    rays_o, rays_d, ray_id, step_id, q, self.scene_center_h, self.scene_radius_h, t_tab, self.bg_len,
                    self.contracted_norm)
            elif self.fused_march:
                raise NotImplementedError('DirectContractedVoxGO(fused_march=True): rays that require grad are not '
                                          'differentiated through the contraction: construct it with raygrad=True')
        return self._render(rays_o, rays_d, viewdirs, stepsize, render_kwargs['bg'], render_kwargs.get('render_depth', False),
                            wrap)

    def _render(self, rays_o, rays_d, viewdirs, stepsize, bg, render_depth, wrap=None):
        """The fused march where the model has it and its records fit, else the sampler and the op-by-op sequence.

        `wrap` (rays that require grad, raygrad=True; None for a plain render): the same launches and the same bits in
        every result key as the forward without, on sample positions that autograd knows as the contraction of their rays
        (ops.contract_points; csrc/contract_raygrad.hip), sampled through the position-differentiable trilinear op
        (csrc/grid_sample_xyz.hip).  On the fused march the density's share of the ray gradient comes from the march's own
        backward, k0's through the wrapped positions.  Stop-gradients, by contract:
          * the table of distances `t` is a constant (so the normalisation of rays_d IS differentiated, unlike
            DirectVoxGO._forward_raygrad's lam);
          * the set of kept samples is fixed: thinning, occupancy and both fast_color_thres filters select rows;
          * `s` and `depth` carry no gradient: the distortion loss reaches the rays through `weights` only;
          * viewdirs carries no gradient (the colour heads have no input gradient for the view embedding).
        At an inf-norm tie the lowest axis index attaining max|p_a| carries the norm's derivative; n == 1 is the identity."""
        N = len(rays_o)
        if self.fused_march:
            cfg = self._march_contract_cfg(stepsize, self.density.device)
            march = fused_march_contract(self.density, rays_o, rays_d, cfg, raygrad=wrap is not None)
            if march is not None:
                weights, alpha, alphainv_last, q, ray_id, step_id, t, _ = march
                rgb = self._colour(q if wrap is None else wrap(q, ray_id, step_id), None, viewdirs, ray_id)
                ret = self._sum_rays(N, weights, alpha, alphainv_last, rgb, ray_id, bg, render_depth, step_id, t)
                ret['n_max'] = cfg.n_max
                return ret
        with torch.no_grad():                                 # the sampler's outputs are constants either way
            q, ray_id, step_id, t, n_max = self.sample_ray(rays_o, rays_d, stepsize)
        ret = self._forward_unfused(N, viewdirs, stepsize, bg, render_depth, q if wrap is None else wrap(q, ray_id, step_id),
                                    ray_id, step_id, t)
        ret['n_max'] = n_max
        return ret

    @property
    def scene_center_h(self):
        """The foreground box's centre as a host array (kernel argument of the ray gradient); read once per device copy."""
        return self._host3('scene_center')

    @property
    def scene_radius_h(self):
        return self._host3('scene_radius')

    def _host3(self, name):
        buf = getattr(self, name)
        key = (name, buf.data_ptr())
        if key not in self._tab_cache:
            self._tab_cache[key] = L.f3(buf)
        return self._tab_cache[key]

    def _sum_rays(self, N, weights, alpha, alphainv_last, rgb, ray_id, bg, render_depth, step_id, t):
        """Per-ray sums in fixed order (the march's composite over the ray offsets): bitwise repeatable renders.  The
        depth is this model's own: it sums `t`, not `step_id`."""
        off = ray_offsets(ray_id, N)
        ret = self._finish_marched(N, weights, alpha, alphainv_last, rgb, ray_id, step_id, off, bg, False)
        ret.update(step_id=step_id, t=t, s=1 - 1 / (1 + t))
        if render_depth:
            with torch.no_grad():
                t3 = t.unsqueeze(-1).expand(-1, 3).contiguous()
                ret['depth'] = composite(weights.detach(), t3, torch.zeros(N, device=weights.device), ray_id, off, 0.0)[:, 0]
        return ret
