"""DirectVoxGO scene model, host side, on the MI355X kernels.

Build-side counterpart of /root/reference/lib/dvgo.py:30-577 for the rows of SURVEY.md
section 8a (H1 sample_ray / hit_coarse_geo, H2 forward): same constructor arguments, same
``state_dict`` keys ('density', 'k0', 'rgbnet.*', 'mask_cache.*', 'xyz_min', 'xyz_max',
'viewfreq'), same ``forward(rays_o, rays_d, viewdirs, global_step, **render_kwargs)`` contract and
result dict, so the training / rendering loops of run.py consume it unchanged.

Two execution paths produce the same dict:
  fused=True   (default) csrc/march.hip: 4 kernels, 1 host sync per forward;
  fused=False  the reference's own op-by-op orchestration on the drop-in ops of
               render_utils.py / ops.py (what a maintainer gets by only swapping the bindings).
Rays that require grad (camera-pose refinement, pose.py) take a third, op-by-op path that is also differentiable with respect
to the rays: `_forward_raygrad`; with the class switch `fused_raygrad` set (pose.refine_poses(fused=True) sets it for its
loop) they stay on the fused march, whose backward then also returns the ray gradients (csrc/march_raygrad.hip: march_ray_bwd).
`posbase_pe=P > 0` (lib/dvgo.py:97-107,528-534, the switch of configs/nerf and configs/nsvf) colours a sample from
the positional encoding of its position instead of the feature grid: the colour head's input is
cat([pts, sin(pts (x) posfreq), cos(pts (x) posfreq), viewdirs_emb]), there is no diffuse term, and k0 -- still allocated,
still in the state_dict -- is neither read nor trained (its .grad stays None, as in the reference).  The fused path runs
the head as csrc/shade_pe.hip (width 128, d_in <= 96) on positions the march writes in place of features.
The fork's other experiments raise NotImplementedError: rgbnet_full_implicit (the reference's own forward reads a k0 it
never assigns, lib/dvgo.py:498-522) and the LIIF option implicit_voxel_feat (lib/dvgo.py:329-410; only the tri-plane
configs set it, and its branches read an undefined k0 or unpack four values into three names, lib/dvgo.py:336).
"""
import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import render_utils as render_utils_hip
from ._lib import _flt, _i64, _int, f3, ptr, stream_of
from .fused import MarchConfig, fused_hit
from .ops import ray_points
from .shade import head_layers
from .voxel_model import (VoxelModel, _check_rays, _freqs, _rays_want_grad,  # noqa: F401 (tests and tools import the last two
                          make_rgbnet, mlp_forward)                        # from here)


class DirectVoxGO(VoxelModel):
    # rays that require grad stay on the fused march (fused.py launches dvgo_march_ray_bwd in the backward) instead of taking
    # `_forward_raygrad`.  A switch of the running process, not of the model: no constructor argument, not in get_kwargs(),
    # not in checkpoints.
    fused_raygrad = False

    def __init__(self, xyz_min, xyz_max, num_voxels=0, num_voxels_base=0, alpha_init=None,
                 mask_cache_path=None, mask_cache_thres=1e-3, fast_color_thres=0,
                 rgbnet_dim=0, rgbnet_direct=False, rgbnet_full_implicit=False,
                 rgbnet_depth=3, rgbnet_width=128, viewbase_pe=4,
                 posbase_pe=0, implicit_voxel_feat=False,
                 channels_last=True, fused=True, verbose=False, **kwargs):
        super().__init__()
        if rgbnet_full_implicit:
            raise NotImplementedError('rgbnet_full_implicit: the reference forward reads k0 before assigning it '
                                      '(lib/dvgo.py:498-522), so there is no behaviour to reproduce')
        if implicit_voxel_feat:
            raise NotImplementedError('implicit_voxel_feat (LIIF) is a tri-plane-only experiment whose dvgo branches are '
                                      'broken in the reference (undefined k0; lib/dvgo.py:336 unpacks 4 values into 3)')
        self.verbose = verbose
        self.fused = bool(fused)
        self.fused_shade = True          # fp32-MFMA colour head (csrc/shade.hip) when the rgbnet has the default shape
        self.channels_last = bool(channels_last)
        self._set_box(xyz_min, xyz_max)
        self.fast_color_thres = fast_color_thres

        # lib/dvgo.py:55-62
        self.num_voxels_base = num_voxels_base
        self.voxel_size_base = ((self._xyz_max_cpu - self._xyz_min_cpu).prod() / self.num_voxels_base).pow(1 / 3)
        self.alpha_init = alpha_init
        self.act_shift = np.log(1 / (1 - alpha_init) - 1)
        self._set_grid_resolution(num_voxels)

        ws = [int(v) for v in self.world_size]
        self.density = nn.Parameter(torch.zeros([1, 1, *ws]))
        self.rgbnet_kwargs = {
            'rgbnet_dim': rgbnet_dim, 'rgbnet_direct': rgbnet_direct,
            'rgbnet_full_implicit': rgbnet_full_implicit,
            'rgbnet_depth': rgbnet_depth, 'rgbnet_width': rgbnet_width, 'viewbase_pe': viewbase_pe,
        }
        # the reference's posbase_pe (lib/dvgo.py:97-107); in get_kwargs() only when set, so that the kwargs and checkpoints of
        # the other models stay as they were
        self.posbase_pe = int(posbase_pe) if rgbnet_dim > 0 else 0
        if posbase_pe > 0:
            self.rgbnet_kwargs['posbase_pe'] = posbase_pe
        if rgbnet_dim > 0:
            self.rgbnet_direct = rgbnet_direct
        # what the MLP reads before the view embedding: the positions' encoding, or the k0 channels that are not diffuse colour
        feat_dim = 3 + 3 * self.posbase_pe * 2 if self.posbase_pe > 0 else rgbnet_dim if rgbnet_direct else rgbnet_dim - 3
        self._init_colour(ws, rgbnet_dim, feat_dim, viewbase_pe, rgbnet_width, rgbnet_depth)
        if self.posbase_pe > 0:
            self.register_buffer('posfreq', _freqs(self.posbase_pe))
        self._init_mask_cache(ws, mask_cache_path, mask_cache_thres)

    # ------------------------------------------------------------------ sizing / bookkeeping
    def _set_grid_resolution(self, num_voxels):
        """lib/dvgo.py:155-165 (float32 tensor maths on the host)."""
        self.num_voxels = num_voxels
        ext = self._xyz_max_cpu - self._xyz_min_cpu
        self.voxel_size = (ext.prod() / num_voxels).pow(1 / 3)
        self.world_size = (ext / self.voxel_size).long()
        self.voxel_size_ratio = self.voxel_size / self.voxel_size_base
        self._cfg_cache = {}
        if self.verbose:
            print('dvgo_amd: world_size', self.world_size.tolist(), 'voxel_size', float(self.voxel_size),
                  'voxel_size_ratio', float(self.voxel_size_ratio))

    def get_kwargs(self):
        return {
            'xyz_min': self._xyz_min_cpu.numpy(), 'xyz_max': self._xyz_max_cpu.numpy(),
            'num_voxels': self.num_voxels, 'num_voxels_base': self.num_voxels_base,
            'alpha_init': self.alpha_init, 'act_shift': self.act_shift,
            'voxel_size_ratio': self.voxel_size_ratio,
            'mask_cache_path': self.mask_cache_path, 'mask_cache_thres': self.mask_cache_thres,
            'fast_color_thres': self.fast_color_thres,
            **self.rgbnet_kwargs,
        }

    # ------------------------------------------------------------------ grid maintenance (N4)
    @torch.no_grad()
    def maskout_near_cam_vox(self, cam_o, near):
        """lib/dvgo.py:215-226: density = -100 wherever a training camera is within `near` (one kernel over the voxels,
        csrc/maintain.hip; the voxel centres are the reference's torch.linspace coordinates)."""
        self._maskout_near_cam(self.density, cam_o, near)

    def _maskout_near_cam(self, grid, cam_o, near):
        """dvgo_maskout_near_cam on `grid` [1,1,X,Y,Z]: -100 at the lattice points of the box within `near` of a camera."""
        dev = grid.device
        X, Y, Z = (int(v) for v in grid.shape[2:])
        gx, gy, gz = (torch.linspace(float(self._xyz_min_cpu[a]), float(self._xyz_max_cpu[a]), n, device=dev)
                      for a, n in enumerate((X, Y, Z)))
        cams = torch.as_tensor(cam_o, dtype=torch.float32).reshape(-1, 3).to(dev).contiguous()
        with L.device_of(grid):
            L.call('dvgo_maskout_near_cam', ptr(grid), ptr(gx), ptr(gy), ptr(gz), _int(X), _int(Y), _int(Z),
                   ptr(cams), _int(cams.shape[0]), _flt(float(near)), _flt(-100.0), stream_of(grid))

    @torch.no_grad()
    def scale_volume_grid(self, num_voxels):
        """Progressive up-scaling (lib/dvgo.py:228-263)."""
        self._set_grid_resolution(num_voxels)
        ws = self._resize_grids()
        mask = self._alpha_mask()
        if self.mask_cache_path:
            mask = self._coarse_mask(ws, self.density.device) & mask
        self._set_mask_cache(mask)

    @torch.no_grad()
    def voxel_count_views(self, rays_o_tr, rays_d_tr, imsz, near, far, stepsize, downrate=1, irregular_shape=False):
        """How many training views see each voxel (lib/dvgo.py:265-295; drives the coarse stage's per-voxel learning
        rate, run.py:311-320).  The reference pushes ones through grid_sample and reads `ones.grad > 1` per view; here
        the per-view weight sums are accumulated by one kernel (one wavefront per ray) and committed by another
        (csrc/maintain.hip) -- same argument meaning, returns count [1,1,X,Y,Z] float."""
        dev = self.density.device
        X, Y, Z = (int(v) for v in self.density.shape[2:])
        n_samples = int(np.linalg.norm(np.array([X, Y, Z]) + 1) / stepsize) + 1
        step = float(np.float32(stepsize) * self.voxel_size.numpy().astype(np.float32))
        count = torch.zeros_like(self.density.detach())
        acc = torch.zeros(X * Y * Z, dtype=torch.float32, device=dev)
        mn, mx = f3(self._xyz_min_cpu), f3(self._xyz_max_cpu)
        with L.device_of(self.density):
            st = stream_of(self.density)
            for rays_o_, rays_d_ in zip(rays_o_tr.split(imsz), rays_d_tr.split(imsz)):
                if not irregular_shape:
                    rays_o_, rays_d_ = rays_o_[::downrate, ::downrate], rays_d_[::downrate, ::downrate]
                ro = rays_o_.to(dev).reshape(-1, 3).float().contiguous()
                rd = rays_d_.to(dev).reshape(-1, 3).float().contiguous()
                L.call('dvgo_view_weight_accumulate', ptr(ro), ptr(rd), _i64(ro.shape[0]), mn, mx, _flt(float(near)),
                       _flt(float(far)), _flt(step), _int(n_samples), _int(X), _int(Y), _int(Z), ptr(acc), st)
                L.call('dvgo_view_count_commit', ptr(acc), ptr(count), _i64(X * Y * Z), st)
        return count

    def hit_coarse_geo(self, rays_o, rays_d, near, far, stepsize, **render_kwargs):
        """Rays with at least one sample in known-occupied space (lib/dvgo.py:412-423)."""
        shape = rays_o.shape[:-1]
        rays_o = rays_o.reshape(-1, 3).contiguous()
        rays_d = rays_d.reshape(-1, 3).contiguous()
        if self.fused and self.mask_cache is not None:
            return fused_hit(rays_o, rays_d, self._march_cfg(near, far, stepsize)).reshape(shape)
        stepdist = stepsize * self.voxel_size
        ray_pts, mask_outbbox, ray_id = render_utils_hip.sample_pts_on_rays(
            rays_o, rays_d, self.xyz_min, self.xyz_max, near, far, stepdist)[:3]
        mask_inbbox = ~mask_outbbox
        hit = torch.zeros([len(rays_o)], dtype=torch.bool, device=rays_o.device)
        hit[ray_id[mask_inbbox][self.mask_cache(ray_pts[mask_inbbox])]] = 1
        return hit.reshape(shape)

    def sample_ray(self, rays_o, rays_d, near, far, stepsize, is_train=0, **render_kwargs):
        """lib/dvgo.py:425-448 -> (ray_pts, ray_id, step_id) of the in-box samples, near to far."""
        rays_o = rays_o.contiguous()
        rays_d = rays_d.contiguous()
        stepdist = stepsize * self.voxel_size
        ray_pts, mask_outbbox, ray_id, step_id, N_steps, t_min, t_max = render_utils_hip.sample_pts_on_rays(
            rays_o, rays_d, self.xyz_min, self.xyz_max, near, far, stepdist)
        mask_inbbox = ~mask_outbbox
        return ray_pts[mask_inbbox], ray_id[mask_inbbox], step_id[mask_inbbox]

    # ------------------------------------------------------------------ ray gradients (camera-pose refinement, pose.py)
    def forward(self, rays_o, rays_d, viewdirs, global_step=None, **render_kwargs):
        """VoxelModel.forward; with grad mode on and `rays_o` or `rays_d` requiring grad (this class only, posbase_pe == 0,
        whatever `self.fused` says) the render is also differentiable with respect to the rays: see `_forward_raygrad`.
        With `fused_raygrad` set on a fused model such rays take the fused forward instead, rays attached and `viewdirs`
        detached: the same stop-gradients, the derivative from the march's own backward."""
        if _rays_want_grad(rays_o, rays_d) and type(self) is DirectVoxGO and self.posbase_pe == 0:
            if self.fused_raygrad and self.fused and not self.uses_posenc:
                return super().forward(rays_o, rays_d, viewdirs.detach(), global_step=global_step, **render_kwargs)
            return self._forward_raygrad(rays_o, rays_d, viewdirs, **render_kwargs)
        return super().forward(rays_o, rays_d, viewdirs, global_step=global_step, **render_kwargs)

    def _forward_raygrad(self, rays_o, rays_d, viewdirs, near, far, stepsize, bg, render_depth=False, feats=None, **_unused):
        """The op-by-op forward on positions that autograd knows as o + d * lam (ops.ray_points), sampled through the
        position-differentiable trilinear op (csrc/grid_sample_xyz.hip).  Forward values are those of the `fused=False`
        path: the positions are the sampling kernel's own, bit for bit.  Stop-gradients, by contract:
          * lam = t_min[ray_id] + stepdist * step_id / |rays_d[ray_id]| is a constant: neither the box entry t_min nor the
            norm passes a gradient back to the ray;
          * the set of kept samples is fixed: the in-box test, the occupancy mask and both fast_color_thres filters select
            rows and are not differentiated;
          * viewdirs carries no gradient (the colour heads have no input gradient for the view embedding).
        `feats`: what the caller handed to a subclass's `render`, passed on to `_forward_unfused` (None: the model's own
        tensors)."""
        _check_rays(rays_o)
        rays_o, rays_d = rays_o.contiguous(), rays_d.contiguous()
        stepdist = stepsize * self.voxel_size
        with torch.no_grad():
            ray_pts, mask_outbbox, ray_id, step_id, _, t_min, _ = render_utils_hip.sample_pts_on_rays(
                rays_o, rays_d, self.xyz_min, self.xyz_max, near, far, stepdist)
            keep = ~mask_outbbox
            ray_pts, ray_id, step_id = ray_pts[keep], ray_id[keep], step_id[keep]
            if self.mask_cache is not None:
                keep = self.mask_cache(ray_pts)
                ray_pts, ray_id, step_id = ray_pts[keep], ray_id[keep], step_id[keep]
            lam = t_min[ray_id] + (float(stepdist) * step_id) / rays_d.norm(dim=-1)[ray_id]
        pts = ray_points(rays_o, rays_d, lam.contiguous(), ray_id, ray_pts.contiguous())
        return self._forward_unfused(len(rays_o), viewdirs.detach(), stepsize, bg, render_depth, pts, ray_id, step_id, feats=feats)

    # ------------------------------------------------------------------ colour head and forward (H2)
    @property
    def uses_posenc(self):
        """True when the colour head reads the positional encoding of the sample positions and not k0 (posbase_pe > 0,
        fine stage): k0 then gets no gradient and is never updated."""
        return self.rgbnet is not None and self.posbase_pe > 0

    def _march_cfg(self, near, far, stepsize):
        return self._cached_cfg((float(near), float(far), float(stepsize)),
                                lambda: self._new_march_cfg(near, far, stepsize, self.act_shift))

    def _new_march_cfg(self, near, far, stepsize, act_shift):
        return MarchConfig(self.xyz_min, self.xyz_max, stepdist=float(stepsize * self.voxel_size), act_shift=act_shift,
                           interval=float(stepsize * self.voxel_size_ratio), fast_color_thres=self.fast_color_thres,
                           near=near, far=far, **self._mask_args())

    def can_keep_count_on_device(self):
        """True when `forward(..., _capacity=True)` is available: the fused march with the fused colour head."""
        return bool(self.fused and self.fused_shade and self.rgbnet is not None and not self.uses_posenc
                    and head_layers(self.rgbnet) is not None)
