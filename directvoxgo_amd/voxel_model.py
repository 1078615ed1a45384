"""VoxelModel: what the scene models share, once.

A scene model here is a density, colour features (a grid `k0`, planes, a hash table) with an optional shallow MLP behind
them, and an occupancy `mask_cache`, all over one axis-aligned box, volume-rendered along rays.  `VoxelModel` owns the box
buffers and their host copies, grid allocation / resizing / the occupancy mask rebuilt from the grids, the colour head and
its construction, the op wrappers, and the render skeleton:

  `_forward_fused`     fused_march -> colour -> `_finish_marched`;
  `_finish_marched`    how every march ends: composite -> result dict (-> n_samples) (-> composite_depth);
  `_render_unfused`    sample_ray -> occupancy lookup -> `_forward_unfused`;
  `_forward_unfused`   `_raw_density` -> alpha -> alpha filter -> Alphas2Weights -> weight filter -> `_colour` -> `_sum_rays`;
  `_sum_rays`          the per-ray sum, the dict and the depth on segment_coo (DirectVoxGO, DirectMPIGO);
  `_sum_rays_in_order` the same in the marches' fixed order: offsets from the sorted ray_id, then `_finish_marched`;
  `_cached_cfg`        the march-config cache behind every config builder; `_set_mask_cache` empties it;
  `_check_rays`, `_rays_want_grad`   the two predicates of every forward and render.

Hooks, with this class's grids as the default: `_raw_density(pts, feats)` (the density grid) and `_colour(pts, feats,
viewdirs, ray_id)` (k0, or the positions' encoding under `uses_posenc`).  A subclass still owns its constructor,
`_set_grid_resolution`, `get_kwargs`, `sample_ray`, its config builder (`_march_cfg` and its kin), its maintenance kernels,
which march its `forward` / `render` calls and which `_sum_rays` it ends in; see dvgo.py (bounded scenes), dmpigo.py (NDC /
multi-plane), dcvgo.py (contracted space) and triplane.py with its subclasses (features from planes, lines or a hash table).
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .fused import composite, composite_depth, fused_march
from .ops import Alphas2Weights, MaskCache, Raw2Alpha, grid_sample, ray_offsets, segment_coo, total_variation_add_grad
from .shade import shade, shade_posenc, viewdir_embed


def _as_f32(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float32) if not isinstance(x, torch.Tensor) else x.detach().cpu(),
                           dtype=torch.float32)


class _LinearSplitK(torch.autograd.Function):
    """y = x @ W^T + b for tall-skinny x [M, K] (M ~ 10^6 samples, K, N <= 128).

    Same maths as nn.Linear; only the weight gradient is evaluated differently: dW = g^T x is a
    reduction over the M samples into a tiny [N, K] output, for which the stock GEMM picks a
    3-ms single-pass kernel at M = 2 M (profiles/r1).  Here the samples are cut into chunks that are
    reduced as one batched GEMM (parallel over chunks) and then summed."""
    CHUNK = 8192

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        return torch.addmm(bias, x, weight.t())

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        g = g.contiguous()
        gx = g @ weight if ctx.needs_input_grad[0] else None
        M, chunk = x.shape[0], _LinearSplitK.CHUNK
        main = (M // chunk) * chunk
        gw = None
        if main:
            S = main // chunk
            gw = torch.bmm(g[:main].view(S, chunk, -1).transpose(1, 2), x[:main].view(S, chunk, -1)).sum(0)
        if main < M:
            tail = g[main:].t() @ x[main:]
            gw = tail if gw is None else gw + tail
        return gx, gw, g.sum(0)


def mlp_forward(net, x):
    """Run an rgbnet (nn.Sequential of Linear / ReLU / nested Sequential) with the split-K linear for
    large sample counts; identical module tree and parameters."""
    for mod in net:
        if isinstance(mod, nn.Sequential):
            x = mlp_forward(mod, x)
        elif isinstance(mod, nn.Linear) and x.shape[0] >= 4 * _LinearSplitK.CHUNK and x.requires_grad | mod.weight.requires_grad:
            x = _LinearSplitK.apply(x.contiguous(), mod.weight, mod.bias)
        else:
            x = mod(x)
    return x


def make_rgbnet(dim0, width, depth):
    """Same module tree (hence state_dict keys) as lib/dvgo.py:123-131."""
    net = nn.Sequential(
        nn.Linear(dim0, width), nn.ReLU(inplace=True),
        *[nn.Sequential(nn.Linear(width, width), nn.ReLU(inplace=True)) for _ in range(depth - 2)],
        nn.Linear(width, 3))
    nn.init.constant_(net[-1].bias, 0)
    return net


def _freqs(n):
    return torch.FloatTensor([(2 ** i) for i in range(n)])


def _posenc(x, freq):
    """cat([x, sin(x (x) freq), cos(x (x) freq)]) over the last axis (lib/dvgo.py:524-525,530-531), in torch ops."""
    emb = (x.unsqueeze(-1) * freq).flatten(-2)
    return torch.cat([x, emb.sin(), emb.cos()], -1)


def _result(alphainv_last, weights, rgb_marched, alpha, rgb, ray_id):
    """The reference's result dict (lib/dvgo.py:560-567)."""
    return {'alphainv_last': alphainv_last, 'weights': weights, 'rgb_marched': rgb_marched,
            'raw_alpha': alpha, 'raw_rgb': rgb, 'ray_id': ray_id}


def _check_rays(rays_o):
    assert len(rays_o.shape) == 2 and rays_o.shape[-1] == 3, 'Only suuport point queries in [N, 3] format'


def _rays_want_grad(rays_o, rays_d):
    """True when a render has to be differentiable with respect to its rays."""
    return torch.is_grad_enabled() and (rays_o.requires_grad or rays_d.requires_grad)


class VoxelModel(nn.Module):
    """Base of DirectVoxGO, DirectMPIGO and DirectContractedVoxGO (see the module docstring).

    A subclass constructor calls, in this order (it is the order of the state_dict): `_set_box`, its own
    `_set_grid_resolution`, creates `density`, then `_init_colour` and `_init_mask_cache` / `_set_mask_cache`.  It sets
    `fused`, `fused_shade`, `channels_last`, `fast_color_thres`, `act_shift`, `voxel_size_ratio` and `world_size`."""

    rgbnet_direct = True     # the MLP reads every k0 channel and there is no diffuse term, unless an instance says otherwise
    uses_posenc = False      # True when the colour head reads the samples' positions and not k0 (DirectVoxGO, posbase_pe > 0)

    def can_keep_count_on_device(self):
        """True when `forward(..., _capacity=True)` is available (the sample count stays on the device)."""
        return False

    # ------------------------------------------------------------------ box
    def _set_box(self, xyz_min, xyz_max):
        """The grids' box as buffers, and host copies: sizing maths runs on the CPU in float32 exactly like the
        reference's tensor expressions, and never costs a device sync afterwards."""
        xyz_min, xyz_max = _as_f32(xyz_min), _as_f32(xyz_max)
        self.register_buffer('xyz_min', xyz_min.clone())
        self.register_buffer('xyz_max', xyz_max.clone())
        self._xyz_min_cpu, self._xyz_max_cpu = xyz_min.clone(), xyz_max.clone()

    # ------------------------------------------------------------------ grids and occupancy
    def _alloc_k0(self, ws, device=None):
        g = torch.zeros([1, self.k0_dim, *ws], device=device)
        if self.channels_last and self.k0_dim > 1:
            g = g.contiguous(memory_format=torch.channels_last_3d)
        return g

    def _grid_xyz(self, ws, device):
        return torch.stack(torch.meshgrid(
            *[torch.linspace(float(self._xyz_min_cpu[a]), float(self._xyz_max_cpu[a]), ws[a], device=device)
              for a in range(3)], indexing='ij'), -1)

    def _resize_grids(self):
        """Both grids trilinearly resized to `world_size` (what every scale_volume_grid does first) -> the new size."""
        ws = tuple(int(v) for v in self.world_size)
        self.density = nn.Parameter(F.interpolate(self.density.data, size=ws, mode='trilinear', align_corners=True))
        k0 = F.interpolate(self.k0.data.contiguous(), size=ws, mode='trilinear', align_corners=True)
        if self.channels_last and self.k0_dim > 1:
            k0 = k0.contiguous(memory_format=torch.channels_last_3d)
        self.k0 = nn.Parameter(k0)
        return ws

    def _pooled_alpha(self):
        """[1,1,X,Y,Z]: the activated density, max-pooled over each voxel's 3^3 neighbourhood."""
        return F.max_pool3d(self.activate_density(self.density), kernel_size=3, padding=1, stride=1)

    def _alpha_mask(self):
        """bool [X,Y,Z]: voxels whose neighbourhood holds an alpha above fast_color_thres (lib/dvgo.py:253-254)."""
        return self._pooled_alpha()[0, 0] > self.fast_color_thres

    def _coarse_mask(self, ws, device):
        """The coarse stage's MaskCache (mask_cache_path) at this model's voxel centres (lib/dvgo.py:143-148).
        Needs the GPU (the lookup is a HIP op)."""
        coarse = MaskCache(path=self.mask_cache_path, mask_cache_thres=self.mask_cache_thres).to(device)
        return coarse(self._grid_xyz(ws, device))

    def _set_mask_cache(self, mask):
        """The occupancy grid over the box, on the device of the box buffers (not every subclass has a `density`)."""
        self.mask_cache = MaskCache(path=None, mask=mask.cpu(), xyz_min=self._xyz_min_cpu,
                                    xyz_max=self._xyz_max_cpu).to(self.xyz_min.device)
        self._cfg_cache = {}

    def _init_mask_cache(self, ws, mask_cache_path, mask_cache_thres):
        """Occupancy grid (lib/dvgo.py:135-153): seeded from a coarse checkpoint when there is one, else all ones."""
        self.mask_cache_path, self.mask_cache_thres = mask_cache_path, mask_cache_thres
        if mask_cache_path:
            mask = self._coarse_mask(ws, torch.device('cuda', torch.cuda.current_device()))
        else:
            mask = torch.ones(ws, dtype=torch.bool)
        self._set_mask_cache(mask)

    # ------------------------------------------------------------------ colour head
    def _init_colour(self, ws, rgbnet_dim, feat_dim, viewbase_pe, rgbnet_width, rgbnet_depth):
        """`k0_dim`, `viewfreq`, `rgbnet` and `k0`: a colour grid when rgbnet_dim <= 0 (lib/dvgo.py:83-87), else a
        feature grid and a shallow MLP (lib/dvgo.py:88-131) whose input is `feat_dim` numbers of the subclass's choosing
        followed by the view embedding."""
        if rgbnet_dim <= 0:
            self.k0_dim, self.rgbnet = 3, None
        else:
            self.k0_dim = rgbnet_dim
            self.register_buffer('viewfreq', _freqs(viewbase_pe))
            self.rgbnet = make_rgbnet(feat_dim + (3 + 3 * viewbase_pe * 2), rgbnet_width, rgbnet_depth)
        self.k0 = nn.Parameter(self._alloc_k0(ws))

    def _fused_head(self, viewdirs):
        return self.fused and self.fused_shade and viewdirs.is_cuda and viewdirs.dim() == 2

    def _shade(self, k0, viewdirs, ray_id, m_dev=None):
        """lib/dvgo.py:512-541 (bilinear / non-implicit branches) and lib/dmpigo.py:246-257 (rgbnet_direct)."""
        if self.rgbnet is None:
            return torch.sigmoid(k0)
        if self.rgbnet_direct:
            k0_view = k0
        else:
            k0_view = k0[:, 3:]
            k0_diffuse = k0[:, :3]
        if self._fused_head(viewdirs):  # fp32-MFMA colour head (csrc/shade.hip): width 64 / 128, d_in <= 40
            rgb = shade(self.rgbnet, k0, viewdir_embed(viewdirs, self.viewfreq), ray_id, diffuse=not self.rgbnet_direct,
                        m_dev=m_dev)
            if rgb is not None:
                return rgb
        assert m_dev is None, 'capacity mode needs the fused colour head'      # (torch ops would run over undefined rows)
        viewdirs_emb = _posenc(viewdirs, self.viewfreq).flatten(0, -2)[ray_id]
        rgb_logit = mlp_forward(self.rgbnet, torch.cat([k0_view, viewdirs_emb], -1))
        if self.rgbnet_direct:
            return torch.sigmoid(rgb_logit)
        return torch.sigmoid(rgb_logit + k0_diffuse)

    def _shade_posenc(self, pts, viewdirs, ray_id):
        """lib/dvgo.py:524-534 (uses_posenc; `posfreq` is the subclass's buffer): rgb from the positions' encoding and the
        view embedding, no diffuse term."""
        if self._fused_head(viewdirs):
            rgb = shade_posenc(self.rgbnet, pts, viewdir_embed(viewdirs, self.viewfreq), ray_id, self.posfreq)
            if rgb is not None:
                return rgb
        viewdirs_emb = _posenc(viewdirs, self.viewfreq).flatten(0, -2)[ray_id]
        return torch.sigmoid(mlp_forward(self.rgbnet, torch.cat([_posenc(pts, self.posfreq), viewdirs_emb], -1)))

    # ------------------------------------------------------------------ op wrappers
    def _tv_weights(self, weight):
        """(wx, wy, wz) of the total-variation kernels (lib/dvgo.py:297-305)."""
        w = weight * float(self.world_size.max()) / 128
        return w, w, w

    def density_total_variation_add_grad(self, weight, dense_mode, x_range=None):
        total_variation_add_grad(self.density, self.density.grad, *self._tv_weights(weight), dense_mode, x_range)

    def k0_total_variation_add_grad(self, weight, dense_mode, x_range=None):
        total_variation_add_grad(self.k0, self.k0.grad, *self._tv_weights(weight), dense_mode, x_range)

    def activate_density(self, density, interval=None):
        """lib/dvgo.py:307-310"""
        interval = interval if interval is not None else self.voxel_size_ratio
        shape = density.shape
        return Raw2Alpha.apply(density.flatten().contiguous(), self.act_shift, interval).reshape(shape)

    def grid_sampler(self, xyz, *grids, **_unused):
        """lib/dvgo.py:312-328 (bilinear branch)."""
        ret = [grid_sample(g, xyz, self.xyz_min, self.xyz_max) for g in grids]
        return ret[0] if len(ret) == 1 else ret

    # ------------------------------------------------------------------ march configs
    def _cached_cfg(self, key, make):
        """The config `make()` built for `key`, rebuilt when its `mask` is no longer the mask cache's tensor (None when
        there is no mask cache).  `_set_mask_cache` empties the cache."""
        cfg = self._cfg_cache.get(key)
        if cfg is None or cfg.mask is not (self.mask_cache.mask if self.mask_cache is not None else None):
            cfg = self._cfg_cache[key] = make()
        return cfg

    def _mask_args(self):
        """The occupancy mask with its scale and shift, as every march config takes them (none without a mask cache)."""
        mc = self.mask_cache
        return {} if mc is None else dict(mask=mc.mask, xyz2ijk_scale=mc.xyz2ijk_scale, xyz2ijk_shift=mc.xyz2ijk_shift)

    # ------------------------------------------------------------------ hooks
    def _raw_density(self, pts, feats=None):
        """The raw density at `pts` on the op-by-op path: the density grid (a subclass whose density is not a grid says
        its own; `feats` is whatever the caller handed to `render`)."""
        return self.grid_sampler(pts, self.density)

    def _colour(self, pts, feats, viewdirs, ray_id):
        """rgb of the samples at `pts`: from their positions' encoding (uses_posenc), else from k0 there (a subclass whose
        colour features are not k0 says its own).  (The reference also interpolates k0 under posenc and never uses it.)"""
        if self.uses_posenc:
            return self._shade_posenc(pts, viewdirs, ray_id)
        return self._shade(self.grid_sampler(pts, self.k0), viewdirs, ray_id)

    # ------------------------------------------------------------------ forward (H2)
    def forward(self, rays_o, rays_d, viewdirs, global_step=None, **render_kwargs):
        """Volume rendering (lib/dvgo.py:450-577, lib/dmpigo.py:200-283).  Returns the reference's dict:
        alphainv_last [N], weights [M], rgb_marched [N,3], raw_alpha [M], raw_rgb [M,3], ray_id [M]
        (+ depth [N] when render_kwargs['render_depth'])."""
        _check_rays(rays_o)
        if self.fused:
            cfg = self._march_cfg(render_kwargs['near'], render_kwargs['far'], render_kwargs['stepsize'])
            return self._forward_fused(rays_o, rays_d, viewdirs, cfg, **render_kwargs)
        return self._render_unfused(None, rays_o, rays_d, viewdirs, global_step, **render_kwargs)

    def _forward_fused(self, rays_o, rays_d, viewdirs, cfg, bg, render_depth=False, _capacity=False, **_unused):
        """csrc/march.hip: 4 kernels and 1 host sync, then the colour head and the composite.
        `_capacity` (training step only, train.py): no host synchronisation -- the per-sample outputs are allocated at
        their upper bound, only their first `ret['n_samples']` rows (a device scalar) are defined, and every kernel
        downstream reads that count from the device."""
        N = len(rays_o)
        _capacity = bool(_capacity) and self.can_keep_count_on_device() and viewdirs.is_cuda and viewdirs.dim() == 2
        if self.uses_posenc:
            # the march writes the kept samples' positions where it would write their k0 features; k0 is not read
            weights, alpha, alphainv_last, pts, ray_id, step_id, off3 = fused_march(
                self.density, self.k0.detach()[:, :0], rays_o, rays_d, cfg, positions=True)
            m_dev = None
            rgb = self._shade_posenc(pts, viewdirs, ray_id)
        else:
            weights, alpha, alphainv_last, k0, ray_id, step_id, off3 = fused_march(
                self.density, self.k0, rays_o, rays_d, cfg, capacity=_capacity)
            m_dev = off3[N:] if _capacity else None
            rgb = self._shade(k0, viewdirs, ray_id, m_dev)
        return self._finish_marched(N, weights, alpha, alphainv_last, rgb, ray_id, step_id, off3, bg, render_depth, m_dev)

    def _finish_marched(self, N, weights, alpha, alphainv_last, rgb, ray_id, step_id, off3, bg, render_depth, m_dev=None):
        """How every render with per-ray offsets `off3` ends: fused.composite (one ray's samples in order) -> the result
        dict (-> `n_samples`, capacity mode) (-> composite_depth)."""
        ret = _result(alphainv_last, weights, composite(weights, rgb, alphainv_last, ray_id, off3, bg, m_dev), alpha, rgb, ray_id)
        if m_dev is not None:
            ret['n_samples'] = m_dev
        if render_depth:
            ret['depth'] = composite_depth(weights.detach(), step_id, off3, N)
        return ret

    def _render_unfused(self, feats, rays_o, rays_d, viewdirs, global_step=None, **render_kwargs):
        """The reference's op sequence on the drop-in ops (`fused=False`): the sampler, the occupancy lookup, then
        `_forward_unfused`.  `feats`: what the caller handed to a subclass's `render` (None: the model's own tensors)."""
        pts, ray_id, step_id = self.sample_ray(rays_o=rays_o, rays_d=rays_d, is_train=global_step is not None, **render_kwargs)
        if self.mask_cache is not None:                      # skip known free space
            mask = self.mask_cache(pts)
            pts, ray_id, step_id = pts[mask], ray_id[mask], step_id[mask]
        return self._forward_unfused(len(rays_o), viewdirs, render_kwargs['stepsize'], render_kwargs['bg'],
                                     render_kwargs.get('render_depth', False), pts, ray_id, step_id, feats=feats)

    def _forward_unfused(self, N, viewdirs, stepsize, bg, render_depth, pts, ray_id, *carried, feats=None):
        """The reference's op sequence (lib/dvgo.py:470-577) on the drop-in ops, from samples that passed the occupancy
        lookup: `pts`, `ray_id` and whatever other per-sample arrays (`carried`) the subclass's `_sum_rays` wants, all
        taken through the alpha and the weight filter together."""
        alpha = self.activate_density(self._raw_density(pts, feats), stepsize * self.voxel_size_ratio)
        if self.fast_color_thres > 0:
            mask = alpha > self.fast_color_thres
            pts, ray_id, *carried = [x[mask] for x in (pts, ray_id, *carried)]
            alpha = alpha[mask]
        weights, alphainv_last = Alphas2Weights.apply(alpha, ray_id, N)
        if self.fast_color_thres > 0:
            mask = weights > self.fast_color_thres
            weights, alpha = weights[mask], alpha[mask]
            pts, ray_id, *carried = [x[mask] for x in (pts, ray_id, *carried)]
        rgb = self._colour(pts, feats, viewdirs, ray_id)
        return self._sum_rays(N, weights, alpha, alphainv_last, rgb, ray_id, bg, render_depth, *carried)

    def _sum_rays(self, N, weights, alpha, alphainv_last, rgb, ray_id, bg, render_depth, step_id):
        """The per-ray sums of the op-by-op path and its result dict (lib/dvgo.py:554-576): segment_coo, whose summation
        order is its own -- a subclass that sums differently overrides this, nothing here is shared arithmetic."""
        rgb_marched = segment_coo(src=(weights.unsqueeze(-1) * rgb), index=ray_id,
                                  out=torch.zeros([N, 3], device=weights.device), reduce='sum')
        rgb_marched = rgb_marched + alphainv_last.unsqueeze(-1) * bg
        ret = _result(alphainv_last, weights, rgb_marched, alpha, rgb, ray_id)
        if render_depth:
            with torch.no_grad():
                ret['depth'] = segment_coo(src=(weights * step_id), index=ray_id,
                                           out=torch.zeros([N], device=weights.device), reduce='sum')
        return ret

    def _sum_rays_in_order(self, N, weights, alpha, alphainv_last, rgb, ray_id, bg, render_depth, step_id):
        """`_sum_rays` for the subclasses whose two paths agree bit for bit in rgb_marched (lib/tri_dvgo.py:786-808): the
        fused path's own per-ray sum over offsets found in the sorted `ray_id`, in place of segment_coo's atomics."""
        return self._finish_marched(N, weights, alpha, alphainv_last, rgb, ray_id, step_id, ray_offsets(ray_id, N), bg,
                                    render_depth)
