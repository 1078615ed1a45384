"""TriPlaneVoxGO: the reference fork's tri-plane scene model (lib/tri_dvgo.py:36-809), bilinear path, on the MI355X kernels.

The density grid stays 3-D; colour features come from three 2-D feature planes.  Each plane is sampled bilinearly at two
of a sample's three coordinates and the three results are concatenated (`tri_aggregation='concat'`, 3 * rgbnet_dim
features) or summed ('sum', rgbnet_dim features) -- lib/tri_dvgo.py:456-469, here one HIP op (ops.triplane_sample,
csrc/triplane.hip) -- and feed the shallow MLP exactly as k0 features do in DirectVoxGO (lib/tri_dvgo.py:746-783).

Axis mapping (the reference's own: its ind_norm is the flipped coordinate triple and grid_sample's first grid component
addresses W):   plane 'xy': rows y, columns z;   'yz': rows x, columns y;   'zx': rows z, columns x.

In the reference the planes come out of an image encoder per call (`encode_feat`); the encoder, its `Mapping` network and
the pose anchors are not part of this model.  `render(feats, ...)` takes such planes from the caller, gradients flow
into them; `forward(...)` renders the model's own planes, `self.planes` (an nn.ParameterDict, zero-initialised, trained
through `lrate_planes`).  There is no k0, as in the reference.

Regulariser: `plane_regularizers_add_grad` adds the total-variation gradient of the three planes to their `.grad` in one
HIP launch (ops.plane_reg_add_grad, csrc/plane_tv.hip); TrainStep calls it for the config key `weight_tv_planes` inside the
usual tv_after / tv_before / tv_every window.  No default weight is proposed: none has been tuned on this model.

Two execution paths produce the same dict and call the same sampler on bit-equal positions:
  fused=True   fused_march(positions=True) -> triplane_sample -> colour head -> composite;
  fused=False  the reference's op sequence on the drop-in ops.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .dvgo import DirectVoxGO
from .fused import fused_march
from .ops import PLANE_KEYS, plane_reg_add_grad, triplane_sample
from .train import FINE_TRAIN
from .voxel_model import VoxelModel, _check_rays, _freqs, make_rgbnet

# which world axis the rows (H) and the columns (W) of each plane follow
PLANE_AXES = {'xy': (1, 2), 'yz': (0, 1), 'zx': (2, 0)}

# configs/tri_default.py's fine stage on this model: the planes are trained like the feature grid they replace
TRI_FINE_TRAIN = dict(FINE_TRAIN, lrate_planes=1e-1, skip_zero_grad_fields=['density'])

_OUT_OF_SCOPE = {
    'implicit_voxel_feat': 'this class is the bilinear path without a decoder; the plane decoders (Interp_MLP per plane) are '
                           'liif.LIIFTriPlaneVoxGO (liif=True) and interp.InterpTriPlaneVoxGO (liif=False)',
    'liif': 'LIIF local-ensemble decoding belongs to implicit_voxel_feat: liif.LIIFTriPlaneVoxGO',
    'feat_unfold': 'the 3x3 feature unfolding belongs to implicit_voxel_feat and is not built',
    'cell_decode': 'cell decoding belongs to implicit_voxel_feat: liif.LIIFTriPlaneVoxGO, interp.InterpTriPlaneVoxGO',
    'global_cell_decode': 'appending the cell size to the features is not built',
    'feat_fourier': 'the Fourier embedding of the features is not built',
    'feat_pe': 'the positional encoding of the features (feat_fourier) is not built',
    'rgbnet_full_implicit': 'the reference forward reads k0 before assigning it (lib/tri_dvgo.py:728-752): no behaviour to reproduce',
}


class TriPlaneVoxGO(DirectVoxGO):
    """A VoxelModel (through DirectVoxGO, whose sampler, march configuration, occupancy and density maintenance it keeps)
    without k0: the colour features are `triplane_sample(planes, pts)`."""

    rgbnet_direct = False
    posbase_pe = 0
    uses_posenc = False
    k0_dim = 0

    def __init__(self, xyz_min, xyz_max, num_voxels=0, num_voxels_base=0, alpha_init=None,
                 mask_cache_path=None, mask_cache_thres=1e-3, fast_color_thres=0,
                 rgbnet_dim=6, rgbnet_direct=False, rgbnet_depth=3, rgbnet_width=128, viewbase_pe=4,
                 tri_aggregation='concat', plane_size=None, channels_last=True, fused=True, verbose=False, **kwargs):
        VoxelModel.__init__(self)
        for key, why in _OUT_OF_SCOPE.items():
            if kwargs.get(key):
                raise NotImplementedError(f'{key}: {why}')
        if kwargs.get('posbase_pe', 0) > 0 and (kwargs.get('cat_posemb') or kwargs.get('no_voxel_feat')):
            raise NotImplementedError('cat_posemb / no_voxel_feat with posbase_pe > 0: the positional embedding beside or '
                                      'instead of the plane features is not built')
        for key in ('name', 'n_feats', 'n_resblocks', 'pretrained_state_dict', 'map_depth', 'map_width'):
            if key in kwargs:
                raise NotImplementedError(f'{key}: the image encoder, its Mapping network and the pose anchors are not part '
                                          'of this model; pass their planes to render(feats, ...)')
        if rgbnet_dim <= 0:
            raise NotImplementedError('rgbnet_dim <= 0: the reference has no colour-only tri-plane model (lib/tri_dvgo.py:189-190)')
        if tri_aggregation not in ('concat', 'sum'):
            raise ValueError(f"tri_aggregation must be 'concat' or 'sum', got {tri_aggregation!r}")
        self.verbose = verbose
        self.fused = bool(fused)
        self.fused_shade = True
        self.channels_last = bool(channels_last)
        self._set_box(xyz_min, xyz_max)
        self.fast_color_thres = fast_color_thres

        # lib/tri_dvgo.py:124-134
        self.num_voxels_base = num_voxels_base
        self.voxel_size_base = ((self._xyz_max_cpu - self._xyz_min_cpu).prod() / self.num_voxels_base).pow(1 / 3)
        self.alpha_init = alpha_init
        self.act_shift = np.log(1 / (1 - alpha_init) - 1)
        self._set_grid_resolution(num_voxels)
        ws = [int(v) for v in self.world_size]
        self.density = self._alloc_density(ws)

        self.tri_aggregation = tri_aggregation
        self.rgbnet_dim = int(rgbnet_dim)
        self.rgbnet_direct = bool(rgbnet_direct)
        self.plane_size = None if plane_size is None else (int(plane_size[0]), int(plane_size[1]))
        self.rgbnet_kwargs = {
            'rgbnet_dim': rgbnet_dim, 'rgbnet_direct': rgbnet_direct, 'rgbnet_depth': rgbnet_depth,
            'rgbnet_width': rgbnet_width, 'viewbase_pe': viewbase_pe,
        }
        # lib/tri_dvgo.py:200-223: the feature width, and what of it the MLP reads before the view embedding
        self.feat_dim = self._feature_width()
        if not self.rgbnet_direct and self.feat_dim < 3:
            raise ValueError('rgbnet_direct=False takes the first three feature channels as diffuse colour: needs at least 3')
        self._init_head(self.feat_dim if self.rgbnet_direct else self.feat_dim - 3, viewbase_pe, rgbnet_width, rgbnet_depth)
        self.planes = nn.ParameterDict({k: nn.Parameter(self._alloc_plane(self._plane_hw(k))) for k in PLANE_KEYS})
        self._init_mask_cache(ws, mask_cache_path, mask_cache_thres)

    # ------------------------------------------------------------------ construction
    def _init_head(self, mlp_feat_dim, viewbase_pe, rgbnet_width, rgbnet_depth):
        self.register_buffer('viewfreq', _freqs(viewbase_pe))
        self.rgbnet = make_rgbnet(mlp_feat_dim + (3 + 3 * viewbase_pe * 2), rgbnet_width, rgbnet_depth)

    def _alloc_density(self, ws):
        """What the constructor assigns to `density`: the dense grid [1,1,X,Y,Z] (a subclass whose density is not a grid
        creates its own parameters here and returns None)."""
        return nn.Parameter(torch.zeros([1, 1, *ws]))

    def _feature_width(self):
        """What `sample_planes` emits per sample (a subclass with another feature pipeline says its own)."""
        return 3 * self.rgbnet_dim if self.tri_aggregation == 'concat' else self.rgbnet_dim

    def _plane_hw(self, key):
        """(H, W) of plane `key`: `plane_size`, else the two world_size extents its rows and columns follow."""
        if self.plane_size is not None:
            return self.plane_size
        ah, aw = PLANE_AXES[key]
        return int(self.world_size[ah]), int(self.world_size[aw])

    def _alloc_plane(self, hw, device=None):
        p = torch.zeros([1, self.rgbnet_dim, *hw], device=device)
        return p.contiguous(memory_format=torch.channels_last) if self.channels_last else p

    def get_kwargs(self):
        kw = super().get_kwargs()
        kw.update(tri_aggregation=self.tri_aggregation, plane_size=self.plane_size)
        return kw

    # ------------------------------------------------------------------ grid maintenance
    @torch.no_grad()
    def scale_volume_grid(self, num_voxels):
        """lib/tri_dvgo.py:372-407 (density and occupancy), plus the model's own planes: resized with the grid, bilinear
        with align_corners=True, when they take their sizes from world_size; left alone under a fixed `plane_size`."""
        self._set_grid_resolution(num_voxels)
        ws = tuple(int(v) for v in self.world_size)
        self._resize_density(ws)
        if self.plane_size is None:
            for k in PLANE_KEYS:
                p = F.interpolate(self.planes[k].data.contiguous(), size=self._plane_hw(k), mode='bilinear', align_corners=True)
                if self.channels_last:
                    p = p.contiguous(memory_format=torch.channels_last)
                self.planes[k] = nn.Parameter(p)
        mask = self._alpha_mask()
        if self.mask_cache_path:
            mask = self._coarse_mask(ws, self.xyz_min.device) & mask
        self._set_mask_cache(mask)

    def _resize_density(self, ws):
        """The density at the new `world_size` (the counterpart of `_alloc_density`)."""
        self.density = nn.Parameter(F.interpolate(self.density.data, size=ws, mode='trilinear', align_corners=True))

    def k0_total_variation_add_grad(self, weight, dense_mode, x_range=None):
        raise NotImplementedError('k0_total_variation_add_grad: the tri-plane model has no k0 (the reference method reads an '
                                  'attribute it never assigns, lib/tri_dvgo.py:446-449)')

    def _plane_reg_items(self, weight_tv_planes, weight_tv_lines, weight_l1_lines):
        """[(parameter, (wh, ww, wl1))] of the tensors with a non-zero weight.  The normalisation mirrors `_tv_weights`
        (lib/dvgo.py:297-305) and the 3-D kernel's division by its neighbour count, 6: a plane has 4 neighbours, a line 2."""
        if weight_tv_lines != 0 or weight_l1_lines != 0:
            raise ValueError(f'weight_tv_lines / weight_l1_lines: {type(self).__name__} has no lines')
        if weight_tv_planes == 0:
            return []
        items = []
        for k in PLANE_KEYS:
            p = self.planes[k]
            w = weight_tv_planes * max(p.shape[2], p.shape[3]) / 128 / 4
            items.append((p, (w, w, 0.0)))
        return items

    def plane_regularizers_add_grad(self, dense_mode, weight_tv_planes=0.0, weight_tv_lines=0.0, weight_l1_lines=0.0):
        """Total variation on the model's own planes, added to their `.grad` in one launch (ops.plane_reg_add_grad;
        INTEGRATION.md section 6e): wh = ww = weight_tv_planes * max(H, W) / 128 / 4 per plane.  `dense_mode` False: only
        texels whose gradient is non-zero are touched, and a plane without a `.grad` is skipped; True: every texel, and a
        missing `.grad` is created as zeros with the parameter's strides first.  This class has no lines: a non-zero
        line weight is a ValueError.  Planes handed to `render(feats=...)` belong to the caller and are not touched."""
        self._plane_reg_launch(self._plane_reg_items(weight_tv_planes, weight_tv_lines, weight_l1_lines), dense_mode)

    @staticmethod
    def _plane_reg_launch(items, dense_mode):
        """One launch of ops.plane_reg_add_grad for `items` [(parameter, (wh, ww, wl1))], at most 8 of them."""
        params, grads, weights = [], [], []
        for p, w in items:
            if not p.requires_grad:                 # frozen by a zero learning rate: nothing reads its gradient
                continue
            if p.grad is None:
                if not dense_mode:
                    continue
                p.grad = torch.zeros_like(p, memory_format=torch.preserve_format)
            elif p.grad.stride() != p.stride():     # the kernel walks raw memory: the gradient in the parameter's layout
                p.grad = torch.empty_like(p, memory_format=torch.preserve_format).copy_(p.grad)
            params.append(p.detach()); grads.append(p.grad); weights.append(w)
        if params:
            plane_reg_add_grad(params, grads, weights, dense_mode)

    def encode_feat(self, *args, **kwargs):
        raise NotImplementedError('encode_feat: the image encoder, its Mapping network and the pose anchors are not part of '
                                  'this model; pass their planes to render(feats, ...)')

    def can_keep_count_on_device(self):
        return False                 # the sampler sizes its output by the sample count: the forward reads it back

    # ------------------------------------------------------------------ forward
    def forward(self, rays_o, rays_d, viewdirs, global_step=None, **render_kwargs):
        """Renders the model's own planes; see `render`."""
        return self.render(self.planes, rays_o, rays_d, viewdirs, global_step, **render_kwargs)

    def render(self, feats, rays_o, rays_d, viewdirs, global_step=None, **render_kwargs):
        """lib/tri_dvgo.py:688-809.  `feats`: the three planes {'xy', 'yz', 'zx'}, each [1, rgbnet_dim, H, W] (any sizes;
        gradients flow into them).  Returns the reference's dict: alphainv_last [N], weights [M], rgb_marched [N,3],
        raw_alpha [M], raw_rgb [M,3], ray_id [M] (+ depth [N] when render_kwargs['render_depth'])."""
        _check_rays(rays_o)
        if self.fused:
            cfg = self._march_cfg(render_kwargs['near'], render_kwargs['far'], render_kwargs['stepsize'])
            # the march writes the kept samples' positions where it would write k0 features; the stand-in has no channel
            no_k0 = self.density.detach()[:, :0]
            # raygrad='fused' (HashVoxGO, VMTriPlaneVoxGO): rays that require grad stay on this path, the positions carry
            # their gradient back to the march's own ray backward and `viewdirs` carries none
            raygrad = bool(getattr(self, 'raygrad', False) and self.fused_raygrad)
            if raygrad:
                viewdirs = viewdirs.detach()
            weights, alpha, alphainv_last, pts, ray_id, step_id, off3 = fused_march(
                self.density, no_k0, rays_o, rays_d, cfg, positions=True, raygrad=raygrad)
            rgb = self._colour(pts, feats, viewdirs, ray_id)
            return self._finish_marched(len(rays_o), weights, alpha, alphainv_last, rgb, ray_id, step_id, off3,
                                        render_kwargs['bg'], render_kwargs.get('render_depth', False))
        return self._render_unfused(feats, rays_o, rays_d, viewdirs, global_step, **render_kwargs)

    _sum_rays = VoxelModel._sum_rays_in_order      # both paths then agree bit for bit in rgb_marched

    def _colour(self, pts, feats, viewdirs, ray_id):
        return self._shade(self._head_features(pts, feats), viewdirs, ray_id)

    def _head_features(self, pts, feats):
        """What the colour head reads of a sample before the view embedding: the plane features (a subclass may append)."""
        return self.sample_planes(pts, feats)

    def sample_planes(self, pts, feats=None):
        """grid_sampler2D (lib/tri_dvgo.py:456-469): [M, 3 * rgbnet_dim] or, tri_aggregation='sum', [M, rgbnet_dim]."""
        return triplane_sample(self.planes if feats is None else feats, pts, self.xyz_min, self.xyz_max, self.tri_aggregation)
