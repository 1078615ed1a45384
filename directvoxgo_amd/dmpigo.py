"""DirectMPIGO (forward-facing / NDC scenes, BASELINE config 4) on the MI355X kernels.

Host-side counterpart of /root/reference/lib/dmpigo.py:17-290: a multi-plane-image shaped grid
(`mpi_depth` planes along z), a fixed number of samples per ray placed by
``sample_ndc_pts_on_rays`` (K7), ``act_shift = 0`` and ``voxel_size_ratio = 256 / mpi_depth``.
Everything downstream of the sampler is the same op set as DirectVoxGO; the fused path runs the
same four kernels with NDC spacing (include/dvgo_hip.h, `stepdist < 0`).
"""
import numpy as np
import torch
import torch.nn as nn

from . import render_utils as render_utils_hip
from .fused import MarchConfig
from .voxel_model import VoxelModel


class DirectMPIGO(VoxelModel):
    def __init__(self, xyz_min, xyz_max, num_voxels=0, mpi_depth=0, mask_cache_path=None, mask_cache_thres=1e-3,
                 fast_color_thres=0, rgbnet_dim=0, rgbnet_depth=3, rgbnet_width=128, viewbase_pe=0,
                 channels_last=True, fused=True, **kwargs):
        super().__init__()
        self.fused, self.channels_last = bool(fused), bool(channels_last)
        self.fused_shade = True          # fp32-MFMA colour head (csrc/shade.hip) when the rgbnet has a built shape
        self._set_box(xyz_min, xyz_max)
        self.fast_color_thres = fast_color_thres
        self.act_shift = 0
        self._set_grid_resolution(num_voxels, mpi_depth)
        ws = [int(v) for v in self.world_size]

        # density initialised so that every plane has the same stop probability (lib/dmpigo.py:35-44)
        self.density = nn.Parameter(torch.zeros([1, 1, *ws]))
        with torch.no_grad():
            g = np.full([mpi_depth], 1. / mpi_depth - 1e-6)
            p = [1 - g[0]]
            for i in range(1, len(g)):
                p.append((1 - g[:i + 1].sum()) / (1 - g[:i].sum()))
            for i in range(len(p)):
                self.density[..., i].fill_(np.log(p[i] ** (-1 / self.voxel_size_ratio) - 1))
            self.density[..., -1].fill_(10)

        self.rgbnet_kwargs = {'rgbnet_dim': rgbnet_dim, 'rgbnet_depth': rgbnet_depth, 'rgbnet_width': rgbnet_width,
                              'viewbase_pe': viewbase_pe}
        # the MLP reads every k0 channel and there is no diffuse term (lib/dmpigo.py:246-257): VoxelModel's rgbnet_direct
        self._init_colour(ws, rgbnet_dim, rgbnet_dim, viewbase_pe, rgbnet_width, rgbnet_depth)
        self._init_mask_cache(ws, mask_cache_path, mask_cache_thres)

    def _set_grid_resolution(self, num_voxels, mpi_depth):
        """lib/dmpigo.py:97-107"""
        self.num_voxels, self.mpi_depth = num_voxels, mpi_depth
        ext = self._xyz_max_cpu - self._xyz_min_cpu
        r = (num_voxels / self.mpi_depth / ext[:2].prod()).sqrt()
        self.world_size = torch.zeros(3, dtype=torch.long)
        self.world_size[:2] = (ext[:2] * r).long()
        self.world_size[2] = self.mpi_depth
        self.voxel_size_ratio = 256. / mpi_depth
        self._cfg_cache = {}

    def get_kwargs(self):
        return {'xyz_min': self._xyz_min_cpu.numpy(), 'xyz_max': self._xyz_max_cpu.numpy(),
                'num_voxels': self.num_voxels, 'mpi_depth': self.mpi_depth, 'act_shift': self.act_shift,
                'voxel_size_ratio': self.voxel_size_ratio, 'mask_cache_path': self.mask_cache_path,
                'mask_cache_thres': self.mask_cache_thres, 'fast_color_thres': self.fast_color_thres,
                **self.rgbnet_kwargs}

    @torch.no_grad()
    def scale_volume_grid(self, num_voxels, mpi_depth):
        """lib/dmpigo.py:123-146"""
        self._set_grid_resolution(num_voxels, mpi_depth)
        self._resize_grids()
        self._set_mask_cache(self._alpha_mask())

    def _tv_weights(self, weight):
        """lib/dmpigo.py:147-157"""
        wxy = weight * float(self.world_size[:2].max()) / 128
        return wxy, wxy, weight * self.mpi_depth / 128

    def n_samples(self, stepsize):
        return int((self.mpi_depth - 1) / stepsize) + 1          # lib/dmpigo.py:188

    def sample_ray(self, rays_o, rays_d, near, far, stepsize, is_train=False, **render_kwargs):
        """lib/dmpigo.py:173-198"""
        assert near == 0 and far == 1
        N_samples = self.n_samples(stepsize)
        ray_pts, mask_outbbox = render_utils_hip.sample_ndc_pts_on_rays(
            rays_o.contiguous(), rays_d.contiguous(), self.xyz_min, self.xyz_max, N_samples)
        mask_inbbox = ~mask_outbbox
        ray_pts = ray_pts[mask_inbbox]
        dev = rays_o.device
        ray_id = torch.arange(mask_inbbox.shape[0], device=dev).view(-1, 1).expand_as(mask_inbbox)[mask_inbbox]
        step_id = torch.arange(mask_inbbox.shape[1], device=dev).view(1, -1).expand_as(mask_inbbox)[mask_inbbox]
        return ray_pts, ray_id, step_id

    def _march_cfg(self, near, far, stepsize):
        """The fused march with NDC spacing (include/dvgo_hip.h, `stepdist < 0`): a fixed number of samples per ray."""
        assert near == 0 and far == 1
        return self._cached_cfg(float(stepsize), lambda: MarchConfig(
            self.xyz_min, self.xyz_max, stepdist=1.0, act_shift=0.0, interval=float(stepsize * self.voxel_size_ratio),
            fast_color_thres=self.fast_color_thres, near=0.0, far=1.0, ndc_samples=self.n_samples(stepsize),
            **self._mask_args()))
