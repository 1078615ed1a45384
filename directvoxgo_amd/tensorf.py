"""TensoRFVoxGO: VMTriPlaneVoxGO with TensoRF's other half (Chen et al., ECCV 2022, arXiv:2203.09517): the density is
vector-matrix decomposed as well, and no dense density grid exists anywhere in the model.

    raw_density(pts) = sum over the planes xy, yz, zx and their `density_n_comp` components of
                       density_planes[s][r](pts) * density_lines[s][r](pts)                         ops.vm_density
    alpha            = Raw2Alpha(raw_density, act_shift + density_offset, interval)

The sum is one HIP op (csrc/vm_density.hip; include/dvgo_hip.h states the arithmetic and the summation order): the 3 R
products are summed in a register, and the backward scatters one float per sample, so neither direction has an [M, 3R]
intermediate.  Parameters grow with the square of the resolution: 16 components at 640^3 are 79 MB where the dense grid
and its Adam moments are 3 GB.

`density_offset` is a Python float in `get_kwargs`: the progressive-growing schedule subtracts 1 from the dense grid after
every `pg_scale` step (run.py:345), which a sum of products cannot absorb; fit_stage lowers `density_offset` by 1 instead,
as DVGO v2 does through its act_shift.  It costs no launch.

Two render paths give the same dict, bit for bit in everything but the float atomics of the gradient scatter:
  fused_march=False (the default)  op by op: sample_ray -> occupancy lookup -> raw_density -> alpha filter -> Alphas2Weights
      -> weight filter -> sample_planes -> the HIP colour head -> fused.composite / composite_depth.  Every step of every ray
      is materialised, the density is evaluated at every occupied sample, and three boolean compactions each read a count.
  fused_march=True  fused.fused_march_vm (csrc/march_vm.hip: the march of DirectVoxGO with the density taken from planes
      times lines, one wavefront per ray, chunks without an occupied step skipped, nothing behind the ray's stop visited)
      -> sample_planes -> the colour head -> composite.  One host read of two counts (kept samples, records).  Where the
      march has no fixed record stride (an infinite `far`, scratch over the budget) the render takes the first path.
`can_keep_count_on_device()` and `TrainStep.can_capture()` are False on both.

Occupancy goes through `dense_density()`, the op evaluated at the world_size lattice in chunks: `_pooled_alpha`,
`_alpha_mask`, `scale_volume_grid` and fit.compute_bbox_by_coarse_geo read it; it is a temporary, never a parameter.
`maskout_near_cam_vox` cannot write -100 into a grid and clears the occupancy mask at the same voxels instead.

`raygrad=True` (constructor option of the base, default False; not a `get_kwargs` key and not in checkpoints: pass it to the
constructor or to `load_model(TensoRFVoxGO, path, raygrad=True)`): with grad mode on and `rays_o` or `rays_d` requiring grad,
`forward` and `render` take DirectVoxGO._forward_raygrad whatever `fused` and `fused_march` say (the VM march's ray backward
is `raygrad='fused'`, below): the density through `vm_density(..., position_grad=True)`, the features through `vm_sample(...,
position_grad=True) @ basis`, both derivatives one kernel body (csrc/vm_xyz.hip).  Every key of the result has the bits of
the op-by-op forward on the same detached rays; the stop-gradients are `_forward_raygrad`'s.  pose.refine_poses accepts the
model only with this option.

`raygrad='fused'` (the base's: `raygrad` plus the instance attribute `fused_raygrad`; `load_model(TensoRFVoxGO, path,
raygrad='fused')`): with `fused` and `fused_march=True`, rays that require grad stay on the VM march --
`fused_march_vm(..., raygrad=True)`, whose backward launches dvgo_march_vm_ray_bwd (csrc/march_raygrad.hip) first: per
record the raw-density gradient through the position derivative of planes times lines, plus what `vm_sample(...,
position_grad=True) @ basis` returned for the positions, summed per ray; it runs with the model frozen too -- with the
fused march's bits in every key and the same stop-gradients; `viewdirs` is detached.  Without `fused_march`, or where the
march has no fixed record stride, such rays take `_forward_raygrad` as before.  `pose.refine_poses(fused=True)` needs both.

Refused, each naming this class: voxel_count_views / pervoxel_lr, density_total_variation_add_grad (the regularisers of the
density are the config keys train.DENSITY_REG_KEYS), export_volume, extract_mesh, refine_poses and rays that require grad
without `raygrad=True`, data-parallel training, and everything the bases refuse.  Not built: a coarse stage (per-voxel
learning rates), PSNR against a dense density (no quality claim is made), a device-side sample count for the fused march
(its forward reads two counts).  INTEGRATION.md section 6g is the contract.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .fused import fused_march_vm
from .ops import PLANE_KEYS, Raw2Alpha, vm_density
from .triplane import PLANE_AXES
from .voxel_model import _check_rays, _rays_want_grad
from .vm import LINE_AXIS, VM_FINE_TRAIN, VMTriPlaneVoxGO

# VM_FINE_TRAIN with TensoRF's published rate for its grids, 2e-2, on the density planes and lines as well.  The paper's
# numbers, not tuned on this model.  (`lrate_density` stays in the dict and is skipped: the model's `density` is None.)
TENSORF_FINE_TRAIN = dict(VM_FINE_TRAIN, lrate_density_planes=2e-2, lrate_density_lines=2e-2)

# positions per launch of `dense_density`
DENSE_CHUNK = 1 << 22


class TensoRFVoxGO(VMTriPlaneVoxGO):
    """VMTriPlaneVoxGO whose density is `vm_density(density_planes, density_lines, pts)`.  Takes the base's arguments plus
    `density_n_comp` (components per density plane), `density_plane_size` ((H, W) of all three; None: each plane follows
    `world_size` and is resized with it), `density_line_size` (likewise for the three lines), `density_offset` (added
    to act_shift; see the module docstring) and `fused_march` (True: `render` runs on fused.fused_march_vm; default False)."""

    def __init__(self, xyz_min, xyz_max, density_n_comp=16, density_plane_size=None, density_line_size=None,
                 density_offset=0.0, fused_march=False, **kwargs):
        if int(density_n_comp) < 1:
            raise ValueError(f'density_n_comp must be at least 1, got {density_n_comp}')
        if density_line_size is not None and int(density_line_size) < 1:
            raise ValueError(f'density_line_size must be at least 1, got {density_line_size}')
        # read by _alloc_density, which the base constructor calls
        object.__setattr__(self, 'density_n_comp', int(density_n_comp))
        object.__setattr__(self, 'density_plane_size',
                           None if density_plane_size is None else (int(density_plane_size[0]), int(density_plane_size[1])))
        object.__setattr__(self, 'density_line_size', None if density_line_size is None else int(density_line_size))
        object.__setattr__(self, 'density_offset', float(density_offset))
        super().__init__(xyz_min, xyz_max, **kwargs)
        self.fused_march = bool(fused_march)

    # ------------------------------------------------------------------ construction
    def _density_plane_hw(self, key):
        if self.density_plane_size is not None:
            return self.density_plane_size
        ah, aw = PLANE_AXES[key]
        return int(self.world_size[ah]), int(self.world_size[aw])

    def _density_line_n(self, key):
        return self.density_line_size if self.density_line_size is not None else int(self.world_size[LINE_AXIS[key]])

    def _density_tensor(self, shape, device=None):
        t = 0.1 * torch.randn([1, self.density_n_comp, *shape], device=device)       # as the colour planes and lines
        return t.contiguous(memory_format=torch.channels_last) if self.channels_last else t

    def _alloc_density(self, ws):
        """No dense grid: the density planes and lines, and `density` is None (no 'density' key in the state dict)."""
        self.density_planes = nn.ParameterDict(
            {k: nn.Parameter(self._density_tensor(self._density_plane_hw(k))) for k in PLANE_KEYS})
        self.density_lines = nn.ParameterDict(
            {k: nn.Parameter(self._density_tensor((self._density_line_n(k), 1))) for k in PLANE_KEYS})
        return None

    def get_kwargs(self):
        kw = super().get_kwargs()
        kw.update(density_n_comp=self.density_n_comp, density_plane_size=self.density_plane_size,
                  density_line_size=self.density_line_size, density_offset=self.density_offset, fused_march=self.fused_march)
        return kw

    def _refuse(self, what, why):
        raise NotImplementedError(f'{what}: {type(self).__name__} {why}')

    # ------------------------------------------------------------------ density
    def _density_tensors(self, feats):
        """(planes, lines) of a render: the caller's under 'xy_density', ... and 'xy_density_line', ... in `feats`, else the
        model's own."""
        feats = {} if feats is None else feats
        planes = {k: feats[k + '_density'] if k + '_density' in feats else self.density_planes[k] for k in PLANE_KEYS}
        lines = {k: feats[k + '_density_line'] if k + '_density_line' in feats else self.density_lines[k] for k in PLANE_KEYS}
        return planes, lines

    def raw_density(self, pts, feats=None):
        """[...]: the decomposed density at `pts` [..., 3], before the activation.  `feats`: optionally the caller's density
        tensors under 'xy_density', 'yz_density', 'zx_density' and 'xy_density_line', ...; a missing key means the
        model's own tensor.  Gradients flow into whichever is used and, with `raygrad=True`, into positions that require
        grad."""
        planes, lines = self._density_tensors(feats)
        return vm_density(planes, lines, pts, self.xyz_min, self.xyz_max, position_grad=self.raygrad)

    _raw_density = raw_density

    def activate_density(self, density, interval=None):
        """The base's Raw2Alpha with the shift act_shift + density_offset."""
        interval = interval if interval is not None else self.voxel_size_ratio
        shape = density.shape
        return Raw2Alpha.apply(density.flatten().contiguous(), self.act_shift + self.density_offset, interval).reshape(shape)

    @torch.no_grad()
    def dense_density(self, chunk=DENSE_CHUNK):
        """[1,1,X,Y,Z]: `raw_density` at the world_size lattice (the coordinates of `_grid_xyz`), a slab of x at a time so
        that the positions of a launch stay at `chunk`.  A temporary of the caller's: nothing keeps it."""
        dev = self.xyz_min.device
        X, Y, Z = (int(v) for v in self.world_size)
        axes = [torch.linspace(float(self._xyz_min_cpu[a]), float(self._xyz_max_cpu[a]), n, device=dev)
                for a, n in enumerate((X, Y, Z))]
        out = torch.empty([1, 1, X, Y, Z], device=dev)
        rows = max(1, int(chunk) // (Y * Z))
        for x0 in range(0, X, rows):
            xyz = torch.stack(torch.meshgrid(axes[0][x0:x0 + rows], axes[1], axes[2], indexing='ij'), -1)
            out[0, 0, x0:x0 + rows] = self.raw_density(xyz)
        return out

    def _pooled_alpha(self):
        return F.max_pool3d(self.activate_density(self.dense_density()), kernel_size=3, padding=1, stride=1)

    # ------------------------------------------------------------------ grid maintenance
    def _resize_density(self, ws):
        """Density planes and lines that follow world_size, resized like the colour ones (bilinear, align_corners=True);
        fixed sizes are left alone.  Runs before the occupancy mask is rebuilt from `dense_density()`."""
        for params, fixed, size in ((self.density_planes, self.density_plane_size, self._density_plane_hw),
                                    (self.density_lines, self.density_line_size, lambda k: (self._density_line_n(k), 1))):
            if fixed is not None:
                continue
            for k in PLANE_KEYS:
                t = F.interpolate(params[k].data.contiguous(), size=size(k), mode='bilinear', align_corners=True)
                if self.channels_last:
                    t = t.contiguous(memory_format=torch.channels_last)
                params[k] = nn.Parameter(t)

    @torch.no_grad()
    def maskout_near_cam_vox(self, cam_o, near):
        """Where DirectVoxGO writes density = -100 (every lattice point within `near` of a training camera) this model
        clears the occupancy mask: the same kernel on a scratch grid gives the set."""
        scratch = torch.zeros([1, 1, *self.mask_cache.mask.shape], device=self.mask_cache.mask.device)
        self._maskout_near_cam(scratch, cam_o, near)
        self.mask_cache.mask &= scratch[0, 0] != -100

    def voxel_count_views(self, *args, **kwargs):
        self._refuse('voxel_count_views', 'has no per-voxel parameters for a per-voxel learning rate (pervoxel_lr) to act on')

    def density_total_variation_add_grad(self, weight, dense_mode, x_range=None):
        self._refuse('density_total_variation_add_grad',
                     'has no dense density grid; regularise its density planes and lines with the config keys '
                     'weight_tv_density_planes, weight_tv_density_lines, weight_l1_density_planes, weight_l1_density_lines')

    def _density_reg_items(self, weight_tv_density_planes, weight_tv_density_lines, weight_l1_density_planes,
                           weight_l1_density_lines):
        """The six density tensors with the colour side's per-tensor weights: planes wh = ww = tv * max(H, W) / 128 / 4,
        lines wh = tv * N / 128 / 2, and L1 unscaled on either."""
        items = []
        if weight_tv_density_planes != 0 or weight_l1_density_planes != 0:
            for k in PLANE_KEYS:
                p = self.density_planes[k]
                w = weight_tv_density_planes * max(p.shape[2], p.shape[3]) / 128 / 4
                items.append((p, (w, w, weight_l1_density_planes)))
        if weight_tv_density_lines != 0 or weight_l1_density_lines != 0:
            for k in PLANE_KEYS:
                ln = self.density_lines[k]
                items.append((ln, (weight_tv_density_lines * ln.shape[2] / 128 / 2, 0.0, weight_l1_density_lines)))
        return items

    def plane_regularizers_add_grad(self, dense_mode, weight_tv_planes=0.0, weight_tv_lines=0.0, weight_l1_lines=0.0,
                                    weight_tv_density_planes=0.0, weight_tv_density_lines=0.0, weight_l1_density_planes=0.0,
                                    weight_l1_density_lines=0.0):
        """The base's launch for the colour planes and lines, then a second one (a launch takes at most 8 tensors) for the
        density planes and lines."""
        super().plane_regularizers_add_grad(dense_mode, weight_tv_planes, weight_tv_lines, weight_l1_lines)
        self._plane_reg_launch(self._density_reg_items(weight_tv_density_planes, weight_tv_density_lines,
                                                       weight_l1_density_planes, weight_l1_density_lines), dense_mode)

    # ------------------------------------------------------------------ forward
    def _march_vm_cfg(self, near, far, stepsize):
        """The base's MarchConfig (`_march_cfg`, which `hit_coarse_geo` keeps using) with the shift of `activate_density`,
        act_shift + density_offset, formed as it forms it (one float64 sum, narrowed once at the library boundary: the
        same float32).  Cached per (near, far, stepsize, density_offset); `_set_mask_cache` empties the cache."""
        return self._cached_cfg(('vm', float(near), float(far), float(stepsize), self.density_offset),
                                lambda: self._new_march_cfg(near, far, stepsize, self.act_shift + self.density_offset))

    def render(self, feats, rays_o, rays_d, viewdirs, global_step=None, **render_kwargs):
        """The base's result dict from either path of this model (module docstring).  `feats`: the colour planes and
        lines as in the base and, beside them, density tensors under the keys of `raw_density`.  With `raygrad=True`, rays
        that require grad take DirectVoxGO._forward_raygrad on the same `feats`."""
        _check_rays(rays_o)
        want = _rays_want_grad(rays_o, rays_d)
        # raygrad='fused': such rays stay on the VM march (its own ray backward) where this model is on it
        on_march = bool(want and self.raygrad and self.fused_raygrad and self.fused and self.fused_march)
        if self.raygrad and want and not on_march:
            return self._forward_raygrad(rays_o, rays_d, viewdirs, feats=feats, **render_kwargs)
        if self.fused_march:
            if want and not on_march:
                self._refuse('rays that require grad', 'has no derivative of its density with respect to the sample positions: '
                                                       'construct it with raygrad=True')
            cfg = self._march_vm_cfg(render_kwargs['near'], render_kwargs['far'], render_kwargs['stepsize'])
            march = fused_march_vm(*self._density_tensors(feats), rays_o, rays_d, cfg, raygrad=on_march)
            if march is None and on_march:          # no fixed record stride: op by op, as a plain render
                return self._forward_raygrad(rays_o, rays_d, viewdirs, feats=feats, **render_kwargs)
            if march is not None:                   # None: no fixed record stride for these render_kwargs -> op by op
                weights, alpha, alphainv_last, pts, ray_id, step_id, off3 = march
                if on_march:
                    viewdirs = viewdirs.detach()
                rgb = self._colour(pts, feats, viewdirs, ray_id)
                return self._finish_marched(len(rays_o), weights, alpha, alphainv_last, rgb, ray_id, step_id, off3,
                                            render_kwargs['bg'], render_kwargs.get('render_depth', False))
        return self._render_unfused(feats, rays_o, rays_d, viewdirs, global_step, **render_kwargs)
