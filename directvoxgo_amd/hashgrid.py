"""HashVoxGO: DirectVoxGO's density grid with the colour features of a multiresolution hash encoding (Mueller et al.,
Instant-NGP, SIGGRAPH 2022, arXiv:2201.05989), on the MI355X kernels.

The dense `k0` grid carries colour detail at the density lattice's resolution and at its memory cost (12 channels at 256^3:
805 MB before Adam's two moments).  Here the features come from `n_levels` trilinear lattices of growing resolution whose
nodes share one table of rows: a level that fits 2^log2_hashmap_size rows is stored densely, a finer one is hashed into
that many rows (16 levels of 2^19 rows x 2 floats: 64 MB).  The resolutions follow the box, not `world_size`: the table is
not resampled when `scale_volume_grid` grows the density grid.

    features = hash_sample(hash_table, pts)                 [M, n_levels * n_feat]

The sampler and its gradient are one HIP op (ops.hash_sample, csrc/hashgrid.hip; include/dvgo_hip.h states the arithmetic),
read by the usual colour head.  Density stays the dense 3-D grid on the fused march, as in the tri-plane models, whose
`render` (fused march with positions -> sampler -> head -> composite; or the op-by-op sequence with the same per-ray sum)
this class reuses.  No equality with any other implementation is claimed: the contract is INTEGRATION.md section 6f, held
by tests/hash_oracle.py.

`raygrad=True` (constructor option, default False; a plain attribute like DirectContractedVoxGO.raygrad, not a `get_kwargs`
key and not in checkpoints: pass it to the constructor or to `load_model(HashVoxGO, path, raygrad=True)`): with grad mode on
and `rays_o` or `rays_d` requiring grad, `forward` takes DirectVoxGO._forward_raygrad whatever `self.fused` says -- the
sampler's own positions known to autograd as o + d * lam (ops.ray_points), the density through the position-differentiable
trilinear op, the features through `hash_sample(..., position_grad=True)` (csrc/hash_xyz.hip), the per-ray sum the model's
in-order one -- so that pose.refine_poses can move the cameras.  The stop-gradients are `_forward_raygrad`'s (lam constant,
the kept set fixed, no gradient for viewdirs), and every key of the result has the bits of the `fused=False` forward on the
same detached rays (where the fused colour-head kernel takes a `fused=True` model's head, raw_rgb and rgb_marched are that
head's, as in DirectVoxGO._forward_raygrad).  Rays that do not require grad, and every path of a model without the option,
are untouched by it: a default model keeps refusing such rays (fused.fused_march(positions=True) has no ray gradient by default).

`raygrad='fused'` sets `raygrad` and, on the instance, `fused_raygrad` (like `raygrad` no `get_kwargs` key and not in
checkpoints: `load_model(HashVoxGO, path, raygrad='fused')`): with `self.fused`, rays that require grad stay on the fused march
-- `fused_march(positions=True, raygrad=True)`, whose backward launches dvgo_march_ray_bwd_pts (csrc/march_raygrad.hip)
first: the density's share of every record plus what `hash_sample(..., position_grad=True)` returned for the positions,
summed per ray -- with the fused forward's bits in every key and the same stop-gradients; `viewdirs` is detached.  With
`fused=False` such rays take `_forward_raygrad` as before.  `pose.refine_poses(fused=True)` accepts the model only with it.

Left out, each a NotImplementedError naming this class: k0_total_variation_add_grad (no k0), extract_mesh, data-parallel
training, pose refinement without `raygrad=True`, posbase_pe.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .ops import HASH_MAX_LEVELS, HashLevels, hash_sample
from .train import FINE_TRAIN
from .triplane import TriPlaneVoxGO
from .voxel_model import VoxelModel, _rays_want_grad

# FINE_TRAIN with Instant-NGP's published rate for the table, 1e-2.  It is the paper's number and has not been tuned on
# this model.  The table is updated where its gradient is non-zero only, like the density: a row no sample touched in a
# step keeps its value and its moments.
HASH_FINE_TRAIN = dict(FINE_TRAIN, lrate_hash_table=1e-2, skip_zero_grad_fields=['density', 'hash_table'])


def hash_levels(xyz_min, xyz_max, n_levels=16, base_res=16, max_res=512, log2_hashmap_size=19):
    """The level table of a box -> (res int32 [L,3], offsets int64 [L+1]), on the host in float64 from the float32 box:
        s_l      = base_res * (max_res / base_res) ** (l / (L - 1))               (s_0 = base_res when L == 1)
        R_{l,a}  = max(2, floor(s_l * ext_a / max(ext) + 0.5))                    node counts: the longest axis gets s_l
        size_l   = min(Rx * Ry * Rz, 2 ** log2_hashmap_size)                      dense when the nodes fit, else hashed
        offsets  = the running sum of size_l
    It depends on the box only."""
    L_ = int(n_levels)
    if not 1 <= L_ <= HASH_MAX_LEVELS:
        raise ValueError(f'n_levels must be in 1..{HASH_MAX_LEVELS}, got {n_levels}')
    if base_res < 2 or max_res < base_res:
        raise ValueError(f'need 2 <= base_res <= max_res, got base_res={base_res}, max_res={max_res}')
    if not 0 <= int(log2_hashmap_size) <= 31:
        raise ValueError(f'log2_hashmap_size must be in 0..31, got {log2_hashmap_size}')
    mn = np.asarray(torch.as_tensor(xyz_min).detach().cpu().numpy(), np.float32).astype(np.float64)
    mx = np.asarray(torch.as_tensor(xyz_max).detach().cpu().numpy(), np.float32).astype(np.float64)
    ext = mx - mn
    if ext.shape != (3,) or not (ext > 0).all():
        raise ValueError('xyz_max must exceed xyz_min on all three axes')
    res = np.zeros((L_, 3), np.int32)
    offsets = np.zeros(L_ + 1, np.int64)
    for l in range(L_):
        s = float(base_res) * (float(max_res) / float(base_res)) ** (l / (L_ - 1) if L_ > 1 else 0.0)
        r = np.maximum(2, np.floor(s * ext / ext.max() + 0.5)).astype(np.int64)
        res[l] = r
        offsets[l + 1] = offsets[l] + min(int(r[0]) * int(r[1]) * int(r[2]), 1 << int(log2_hashmap_size))
    return torch.from_numpy(res), torch.from_numpy(offsets)


class HashVoxGO(TriPlaneVoxGO):
    """A VoxelModel with DirectVoxGO's density grid, occupancy, sampler and march configuration (through TriPlaneVoxGO,
    whose `render` and per-ray sum it keeps) whose colour features are `hash_sample(hash_table, pts)`; no k0, no planes.
    Takes the density and head arguments of TriPlaneVoxGO plus `n_levels`, `n_feat` (floats per row: 1, 2, 4 or 8),
    `log2_hashmap_size`, `base_res` and `max_res` (nodes along the box's longest axis on the coarsest and the finest level).
    `rgbnet_dim` is not an option: the head reads n_levels * n_feat features."""

    def __init__(self, xyz_min, xyz_max, num_voxels=0, num_voxels_base=0, alpha_init=None,
                 mask_cache_path=None, mask_cache_thres=1e-3, fast_color_thres=0,
                 rgbnet_direct=False, rgbnet_depth=3, rgbnet_width=128, viewbase_pe=4,
                 n_levels=16, n_feat=2, log2_hashmap_size=19, base_res=16, max_res=512,
                 fused=True, verbose=False, raygrad=False, **kwargs):
        VoxelModel.__init__(self)
        if kwargs.pop('posbase_pe', 0):
            raise NotImplementedError('posbase_pe: a positional embedding beside the hash features is not built for HashVoxGO')
        if kwargs:
            raise NotImplementedError(f'{", ".join(sorted(kwargs))}: not an option of HashVoxGO')
        if int(n_feat) not in (1, 2, 4, 8):
            raise ValueError(f'n_feat must be 1, 2, 4 or 8, got {n_feat}')
        if int(n_levels) < 1:
            raise ValueError(f'n_levels must be at least 1, got {n_levels}')
        if max_res < base_res:
            raise ValueError(f'max_res must not be below base_res, got max_res={max_res}, base_res={base_res}')
        self.verbose = verbose
        self.fused = bool(fused)
        self.raygrad = bool(raygrad)              # rays that require grad are differentiated; not in get_kwargs (module docstring)
        if raygrad == 'fused':                    # ... on the fused march where there is one (DirectVoxGO.fused_raygrad, per instance)
            self.fused_raygrad = True
        self.fused_shade = True
        self.channels_last = True
        self._set_box(xyz_min, xyz_max)
        self.fast_color_thres = fast_color_thres

        self.num_voxels_base = num_voxels_base
        self.voxel_size_base = ((self._xyz_max_cpu - self._xyz_min_cpu).prod() / self.num_voxels_base).pow(1 / 3)
        self.alpha_init = alpha_init
        self.act_shift = np.log(1 / (1 - alpha_init) - 1)
        self._set_grid_resolution(num_voxels)
        ws = [int(v) for v in self.world_size]
        self.density = nn.Parameter(torch.zeros([1, 1, *ws]))

        self.n_levels, self.n_feat, self.log2_hashmap_size = int(n_levels), int(n_feat), int(log2_hashmap_size)
        self.base_res, self.max_res = base_res, max_res
        res, offsets = hash_levels(self._xyz_min_cpu, self._xyz_max_cpu, n_levels, base_res, max_res, log2_hashmap_size)
        self.levels = HashLevels(res, offsets)                 # host arrays: they follow from the box and the options
        self.rgbnet_direct = bool(rgbnet_direct)
        self.rgbnet_kwargs = {'rgbnet_direct': rgbnet_direct, 'rgbnet_depth': rgbnet_depth, 'rgbnet_width': rgbnet_width,
                              'viewbase_pe': viewbase_pe}
        self.feat_dim = self.rgbnet_dim = self.n_levels * self.n_feat
        if not self.rgbnet_direct and self.feat_dim < 3:
            raise ValueError('rgbnet_direct=False takes the first three feature channels as diffuse colour: needs '
                             'n_levels * n_feat >= 3')
        self._init_head(self.feat_dim if self.rgbnet_direct else self.feat_dim - 3, viewbase_pe, rgbnet_width, rgbnet_depth)
        # Instant-NGP's initialisation, from torch's global generator
        self.hash_table = nn.Parameter(torch.empty(self.levels.rows, self.n_feat).uniform_(-1e-4, 1e-4))
        self._init_mask_cache(ws, mask_cache_path, mask_cache_thres)

    def get_kwargs(self):
        kw = super(TriPlaneVoxGO, self).get_kwargs()
        kw.update(n_levels=self.n_levels, n_feat=self.n_feat, log2_hashmap_size=self.log2_hashmap_size,
                  base_res=self.base_res, max_res=self.max_res)
        return kw

    # ------------------------------------------------------------------ grid maintenance
    @torch.no_grad()
    def scale_volume_grid(self, num_voxels):
        """The density is resized and the occupancy rebuilt, as in the base; `hash_table` is left alone: its levels follow
        the box, not world_size."""
        self._set_grid_resolution(num_voxels)
        ws = tuple(int(v) for v in self.world_size)
        self.density = nn.Parameter(F.interpolate(self.density.data, size=ws, mode='trilinear', align_corners=True))
        mask = self._alpha_mask()
        if self.mask_cache_path:
            mask = self._coarse_mask(ws, self.density.device) & mask
        self._set_mask_cache(mask)

    def k0_total_variation_add_grad(self, weight, dense_mode, x_range=None):
        raise NotImplementedError('k0_total_variation_add_grad: HashVoxGO has no k0')

    def _plane_reg_items(self, weight_tv_planes, weight_tv_lines, weight_l1_lines):
        if weight_tv_planes != 0 or weight_tv_lines != 0 or weight_l1_lines != 0:
            raise ValueError('weight_tv_planes / weight_tv_lines / weight_l1_lines: HashVoxGO has no planes and no lines')
        return []

    # ------------------------------------------------------------------ forward
    def forward(self, rays_o, rays_d, viewdirs, global_step=None, **render_kwargs):
        """The base's `render` (both paths) on the model's own table; with `raygrad=True`, rays that require grad take
        DirectVoxGO._forward_raygrad (the module docstring says what that means), or, with `raygrad='fused'` on a fused
        model, the base's fused render with the march's own ray backward."""
        if self.raygrad and _rays_want_grad(rays_o, rays_d) and not (self.fused_raygrad and self.fused):
            return self._forward_raygrad(rays_o, rays_d, viewdirs, **render_kwargs)
        return self.render(None, rays_o, rays_d, viewdirs, global_step, **render_kwargs)

    def _head_features(self, pts, feats):
        return self.sample_hash(pts, feats)

    def sample_hash(self, pts, table=None):
        """[M, n_levels * n_feat]; `table`: another table of the model's level layout (gradients flow into it), None: its own.
        With `raygrad=True`, positions that require grad receive theirs."""
        return hash_sample(self.hash_table if table is None else table, pts, self.xyz_min, self.xyz_max, self.levels,
                           position_grad=self.raygrad)

    def sample_planes(self, pts, feats=None):
        raise NotImplementedError('sample_planes: HashVoxGO has no planes; see sample_hash')
