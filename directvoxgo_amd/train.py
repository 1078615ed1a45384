"""Training step of the hot path (harness row H3 of SURVEY.md section 8a) and its ray-parallel
data-parallel form (section 8e).

Counterpart of /root/reference/run.py:348-407: loss terms and weights (:377-386), gradient step
with ``zero_grad(set_to_none=True)`` before backward (:376), optional TV add-grad (:389-395),
MaskedAdam step (:397) and the per-step lr decay (:401-406); optimizer construction follows
lib/utils.py:20-48.

Data parallelism (the reference has none): one process per GPU, rays sharded,
grids / MLP / optimizer state replicated.  Every loss term is normalised by the GLOBAL ray
count so that the sum of the per-rank gradients equals the single-process gradient; the grid
gradients are summed with one all-reduce each (RCCL over xGMI; `backend='nccl'` on ROCm) and
the small MLP gradients travel in one flat bucket.  TV and the masked Adam run after the
reduction because both branch on ``grad != 0`` (total_variation_kernel.cu:21,
adam_upd_kernel.cu:35) and must see the reduced gradient.
"""
import contextlib
import ctypes
from typing import NamedTuple

import torch
import torch.distributed as dist
import torch.nn as nn

from . import _lib as L
from .dp import GridReducer, flat_view  # noqa: F401  (flat_view: part of this module's surface)
from .masked_adam import MaskedAdam
from .fused import brick_union, grid_rows_capture, split_grid_rows
from .shade import defer_wgrad


COARSE_TRAIN = dict(
    N_iters=5000, N_rand=8192, lrate_density=1e-1, lrate_k0=1e-1, lrate_rgbnet=1e-3, lrate_decay=20,
    pervoxel_lr=True, weight_main=1.0, weight_entropy_last=0.01, weight_rgbper=0.1,
    tv_every=1, tv_after=0, tv_before=0, tv_dense_before=0, weight_tv_density=0.0, weight_tv_k0=0.0,
    pg_scale=[], skip_zero_grad_fields=[])            # configs/default.py:36-57
FINE_TRAIN = dict(COARSE_TRAIN, N_iters=20000, pervoxel_lr=False, weight_entropy_last=0.001, weight_rgbper=0.01,
                  pg_scale=[1000, 2000, 3000, 4000], skip_zero_grad_fields=['density', 'k0'])   # :59-68


# optional config keys: total variation on the planes, total variation and L1 on the lines of the tri-plane models
# (model.plane_regularizers_add_grad); read with cfg.get(key, 0.0), inside the tv_after / tv_before / tv_every window,
# divided by the global ray count like weight_tv_density / weight_tv_k0.  No config here sets them: no weight has been tuned
PLANE_REG_KEYS = ('weight_tv_planes', 'weight_tv_lines', 'weight_l1_lines')
# the same for the density planes and lines of a model whose density is decomposed (tensorf.TensoRFVoxGO): total variation
# and L1 on either, read and scaled like PLANE_REG_KEYS and applied by the same method in a second launch
DENSITY_REG_KEYS = ('weight_tv_density_planes', 'weight_tv_density_lines', 'weight_l1_density_planes',
                    'weight_l1_density_lines')


def create_optimizer_or_freeze_model(model, cfg_train, global_step):
    """lib/utils.py:20-48: one param group per `lrate_<name>` whose attribute exists on the model."""
    decay_steps = cfg_train['lrate_decay'] * 1000
    decay_factor = 0.1 ** (global_step / decay_steps)
    groups = []
    for key in cfg_train:
        if not key.startswith('lrate_'):
            continue
        name = key[len('lrate_'):]
        if not hasattr(model, name):
            continue
        param = getattr(model, name)
        if param is None:
            continue
        lr = cfg_train[key] * decay_factor
        if lr > 0:
            if isinstance(param, nn.Module):
                param = param.parameters()
            groups.append({'params': param, 'lr': lr, 'skip_zero_grad': name in cfg_train['skip_zero_grad_fields']})
        elif not isinstance(param, dict):
            param.requires_grad = False
    return MaskedAdam(groups)


def render_loss(render_result, target, n_rays_global, cfg_train):
    """run.py:377-386 with every mean written as sum / global count (identical for one rank)."""
    d = render_result['rgb_marched'] - target
    loss = cfg_train['weight_main'] * d.pow(2).sum() / (3 * n_rays_global)
    if cfg_train['weight_entropy_last'] > 0:
        pout = render_result['alphainv_last'].clamp(1e-6, 1 - 1e-6)
        ent = -(pout * torch.log(pout) + (1 - pout) * torch.log(1 - pout)).sum() / n_rays_global
        loss = loss + cfg_train['weight_entropy_last'] * ent
    if cfg_train['weight_rgbper'] > 0:
        rgbper = (render_result['raw_rgb'] - target[render_result['ray_id']]).pow(2).sum(-1)
        loss = loss + cfg_train['weight_rgbper'] * ((rgbper * render_result['weights'].detach()).sum() / n_rays_global)
    dist_loss = distortion_term(render_result, n_rays_global, cfg_train)
    return loss if dist_loss is None else loss + dist_loss


def distortion_term(render_result, n_rays_global, cfg_train):
    """weight_distortion * distortion_loss (distortion.py) for a result that carries the per-sample `s` (the contracted
    model, dcvgo.py); None otherwise, and for configs without `weight_distortion`."""
    w = cfg_train.get('weight_distortion', 0)
    if not (w > 0 and 's' in render_result):
        return None
    from .distortion import distortion_loss
    return w * distortion_loss(render_result['weights'], render_result['s'], render_result['n_max'],
                               render_result['ray_id'], n_rays_global)


class _FusedLoss(torch.autograd.Function):
    """render_loss in one pass (csrc/loss.hip): the value and d/d{rgb_marched, alphainv_last, raw_rgb}."""
    unit_grad = False        # set by TrainStep around its own loss.backward() (saves three scaling launches)

    @staticmethod
    def forward(ctx, rgb_marched, alphainv_last, raw_rgb, weights, ray_id, target, n_global, w_main, w_ent, w_per, m_dev=None):
        N, M = rgb_marched.shape[0], raw_rgb.shape[0]
        dev = rgb_marched.device
        rgb_marched, alphainv_last, raw_rgb = rgb_marched.contiguous(), alphainv_last.contiguous(), raw_rgb.contiguous()
        g_marched = torch.empty_like(rgb_marched)
        g_last = torch.empty_like(alphainv_last)
        g_raw = torch.empty_like(raw_rgb) if w_per > 0 else None
        loss = torch.empty((), dtype=torch.float32, device=dev)
        with L.device_of(rgb_marched):
            L.call('dvgo_loss_fwd_bwd', rgb_marched, alphainv_last, target.contiguous(), N, raw_rgb, weights.contiguous(), ray_id,
                   M, m_dev, int(n_global), w_main, w_ent, w_per, g_marched, g_last, g_raw, loss, L.stream_of(rgb_marched))
        ctx.save_for_backward(g_marched, g_last, g_raw if g_raw is not None else g_last)
        ctx.has_raw = g_raw is not None
        # rgb_marched = composite(weights, raw_rgb, alphainv_last): the same two tensors reach the loss directly (rgbper,
        # entropy) and through the composite.  When that is the producer of `rgb_marched`, this node's gradients of them
        # are handed to its backward (fused._Composite: `extra`), which adds its own share in place, instead of both being
        # returned to autograd to be summed by two more launches (one of them over [M, 3]).
        fn = rgb_marched.grad_fn
        ctx.partner = None
        if (fn is not None and getattr(fn, 'rgb_ptr', None) == raw_rgb.data_ptr() and getattr(fn, 'last_ptr', None) ==
                alphainv_last.data_ptr() and raw_rgb.requires_grad and alphainv_last.requires_grad):
            ctx.partner = fn
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, go):
        g_marched, g_last, g_raw = ctx.saved_tensors
        unit = _FusedLoss.unit_grad      # TrainStep calls loss.backward() itself: d loss / d loss = 1, nothing to scale
        gm = g_marched if unit else g_marched * go
        gl = g_last if unit else g_last * go
        gr = (g_raw if unit else g_raw * go) if ctx.has_raw else None
        if ctx.partner is not None:
            ctx.partner.extra = (gr, gl)
            ctx.partner = None
            return (gm, None, None, None, None, None, None, None, None, None, None)
        return (gm, gl, gr, None, None, None, None, None, None, None, None)


def fused_render_loss(render_result, target, n_rays_global, cfg_train):
    """Same value and gradients as `render_loss`, one kernel pair instead of ~40 framework launches."""
    return _FusedLoss.apply(render_result['rgb_marched'], render_result['alphainv_last'], render_result['raw_rgb'],
                            render_result['weights'].detach(), render_result['ray_id'], target, n_rays_global,
                            float(cfg_train['weight_main']), float(cfg_train['weight_entropy_last']),
                            float(cfg_train['weight_rgbper']), render_result.get('n_samples'))


class _Plan(NamedTuple):
    """What one step will do, decided once before the forward."""
    path: str            # 'fused' (Adam in the brick kernel) / 'tiles' (the same from all-reduced tiles, if bu.sparse) / 'rows' / 'dense'
    tv: bool             # total variation is added this step
    keep_count: bool     # the sample count stays on the device (model.forward(_capacity=True))


class TrainStep:
    """One optimisation step on one batch of rays; ``world_size > 1`` shards the batch by rank."""

    OVERLAP_MIN_SAMPLES = 600000

    def __init__(self, model, cfg_train, render_kwargs, optimizer=None, process_group=None, fused_loss=True,
                 overlap_wgrad=True, touched_reduce=True, rows_adam=True, track_mse=False, shard_grids=True, sync_free=False):
        self.model = model
        # keep the count of surviving samples on the device (model.forward(_capacity=True)): no host synchronisation in
        # the step.  That is what makes the step capturable (`capture()` switches it on); run eagerly it buys nothing --
        # the sparse step is bound by host work, not by the one read -- and costs capacity-sized temporaries, so it is
        # off by default
        self.sync_free = sync_free
        self._m3_seen = None                 # last sample count read back (asynchronously, a step or two late)
        self._m3_pin, self._m3_event = None, None
        # weight_main * mse of the step, the quantity run.py:378 turns into the logged PSNR (before the entropy and
        # per-point terms are added); kept on the device, no sync
        self.track_mse = track_mse
        self.last_mse = None
        # one GPU, no TV this step: Adam reads the combined gradient rows of the fused backward directly
        # (fused.grid_rows_capture / MaskedAdam.step_grid_rows); density.grad / k0.grad then stay None
        self.rows_adam = rows_adam
        # data parallel, sparse scenes: all-reduce only the voxels some rank touched (see dp.GridReducer._reduce_touched)
        self.touched_reduce = touched_reduce
        self.overlap_wgrad = overlap_wgrad    # colour-head weight gradients on a second stream (shade.defer_wgrad)
        # data parallel, fused HIP model: the grid gradient travels as the tiles of the bricks any rank touched and every
        # rank applies the same fused Adam update (fused.brick_union); used while that union is at most
        # dp.GridReducer.BRICK_SPARSE_MAX (set it on `self.dp`) of the bricks, decided per step from the all-reduced brick counts
        self.brick_sparse = True
        self.last_mode = None                 # 'bricks' / 'sharded' / 'allreduce' / 'touched' / 'single': what the last step used
        self.last_wire_bytes = 0
        self.last_fused_adam = False          # (bench.py: which bytes the scatter launch is credited with)
        self._graph, self._capturing, self._static, self._static_loss = None, False, None, None    # see capture()
        self.fused_loss = fused_loss
        self.cfg = cfg_train
        self.render_kwargs = render_kwargs
        self.optimizer = optimizer or create_optimizer_or_freeze_model(model, cfg_train, global_step=0)
        self.world = dist.get_world_size(process_group) if (dist.is_available() and dist.is_initialized()) else 1
        # a positional-encoding colour head (posbase_pe > 0) reads no k0: only the density grid gets a gradient, so the
        # paths that take both grids' gradients together (brick scatter with the fused Adam, combined gradient rows) stay off
        no_k0 = getattr(model, 'k0', None) is None           # TriPlaneVoxGO: the colour features come from planes, not a grid
        self.k0_idle = bool(getattr(model, 'uses_posenc', False)) or no_k0
        if getattr(model, 'hash_table', None) is not None and self.world > 1:
            raise NotImplementedError(f'data-parallel training of {type(model).__name__} (hash-grid features, a model without '
                                      'k0) is not built: train it on one GPU')
        if getattr(model, 'density_planes', None) is not None and self.world > 1:
            raise NotImplementedError(f'data-parallel training of {type(model).__name__} (decomposed density, no grid to shard '
                                      'or all-reduce) is not built: train it on one GPU')
        if no_k0 and self.world > 1:
            raise NotImplementedError('data-parallel training of a model without k0 (TriPlaneVoxGO) is not built: train it on '
                                      'one GPU')
        if self.k0_idle and self.world > 1:
            raise NotImplementedError('data-parallel training of a posbase_pe model (positional-encoding colour head) is not '
                                      'built: train it on one GPU')
        # the contracted model of unbounded scenes (dcvgo.py) trains on dense grid gradients, op by op or, with its
        # fused_march option, from csrc/march_contract.hip (one raw-density gradient per record, then the grid_sample
        # backward's scatter), and MaskedAdam either way: no brick scatter, no graph capture, no data parallelism
        from .dcvgo import DirectContractedVoxGO
        self.contracted = isinstance(model, DirectContractedVoxGO)
        if self.contracted and self.world > 1:
            raise NotImplementedError('data-parallel training of DirectContractedVoxGO is not built: train it on one GPU')
        # regularisers of plane-shaped parameters (the tri-plane models' planes and lines): optional keys, absent = 0
        self.plane_reg = {k: float(cfg_train.get(k, 0.0)) for k in PLANE_REG_KEYS}
        self.plane_reg_on = any(w > 0 for w in self.plane_reg.values())
        if self.plane_reg_on:
            on = [k for k, w in self.plane_reg.items() if w > 0]
            if not hasattr(model, 'plane_regularizers_add_grad'):
                raise ValueError(f'{", ".join(on)}: {type(model).__name__} has no planes to regularise (the keys belong to the '
                                 'tri-plane models)')
            if not hasattr(model, 'lines') and (self.plane_reg['weight_tv_lines'] > 0 or self.plane_reg['weight_l1_lines'] > 0):
                raise ValueError(f'weight_tv_lines / weight_l1_lines: {type(model).__name__} has no lines (they belong to '
                                 'VMTriPlaneVoxGO)')
        self.density_reg = {k: float(cfg_train.get(k, 0.0)) for k in DENSITY_REG_KEYS}
        self.density_reg_on = any(w > 0 for w in self.density_reg.values())
        if self.density_reg_on and getattr(model, 'density_planes', None) is None:
            on = [k for k, w in self.density_reg.items() if w > 0]
            raise ValueError(f'{", ".join(on)}: {type(model).__name__} has no density planes or lines (they belong to '
                             'TensoRFVoxGO)')
        self.decay_factor = 0.1 ** (1 / (cfg_train['lrate_decay'] * 1000))
        # every collective of the step outside fused.brick_union; None on one GPU
        self.dp = None if self.world == 1 else GridReducer(
            model, self.optimizer, process_group, shard_grids,
            small=[p for n, p in model.named_parameters() if n not in ('density', 'k0') and p.requires_grad])

    def gather_optimizer_state(self):
        """See dp.GridReducer.gather_optimizer_state; no-op (False) on one GPU."""
        return self.dp.gather_optimizer_state() if self.dp is not None else False

    def _sample_count(self, res):
        """Number of surviving samples of the step, without waiting for it: exact when the forward read it back anyway,
        else the last value that has arrived from the device (copied asynchronously into pinned memory every step; no
        host read at all while a graph is being captured)."""
        n_dev = res.get('n_samples')
        if n_dev is None and not self._capturing:
            return res['weights'].shape[0]
        if not self._capturing:
            if self._m3_event is not None and self._m3_event.query():
                self._m3_seen = int(self._m3_pin[0])
            if self._m3_pin is None:
                self._m3_pin = torch.empty(1, dtype=torch.int64).pin_memory()
                self._m3_event = torch.cuda.Event()
            if self._m3_event.query():                 # the previous copy has landed: start the next one
                self._m3_pin.copy_(n_dev, non_blocking=True)
                self._m3_event.record()
        return self._m3_seen if self._m3_seen is not None else res['weights'].shape[0]

    # ------------------------------------------------------------------------------------------------------------
    # HIP-graph replay of the step.  A sparse-scene step is ~45 short kernels (0.55 ms of GPU work at 8192 rays on a
    # lego-like scene) behind ~0.8 ms of host work (Python, allocator, launches): with the sample count kept on the device
    # (`sync_free`) nothing in the step depends on a host read any more, so the whole of it -- forward, loss, backward,
    # grid update inside the brick kernel, MLP Adam -- is captured once and replayed.  What changes from step to step
    # travels through device memory: the batch (copied into the captured input tensors) and the bias-corrected Adam step
    # sizes (`MaskedAdam.hyper_begin`).  Captured: one GPU, fused model + fused colour head, masked Adam on both grids,
    # no total variation, fixed batch size and grid resolution; call `capture()` again after `scale_volume_grid` or an
    # occupancy-mask refresh (both replace tensors the graph holds).
    # ------------------------------------------------------------------------------------------------------------
    def can_capture(self):
        cfg, model = self.cfg, self.model
        density, k0 = getattr(model, 'density', None), getattr(model, 'k0', None)
        tv = self._tv_weighted() and cfg['tv_before'] > cfg['tv_after']
        return bool(self.dp is None and self.fused_loss and self.rows_adam and not tv and not self.k0_idle and not self.contracted
                    and isinstance(self.optimizer, MaskedAdam) and isinstance(density, nn.Parameter) and density.is_cuda
                    and hasattr(model, 'can_keep_count_on_device') and model.can_keep_count_on_device()
                    and self.optimizer.can_fuse_grid_step(density, k0) and self.optimizer.per_lr is None)

    def capture(self, rays_o, rays_d, viewdirs, target, global_step=0, warmup=3):
        """Run `warmup` eager steps on the given batch, then capture one step; later calls with a batch of the same size
        replay it.  Returns False (and stays eager) when the step cannot be captured."""
        self._graph = None
        if not self.can_capture():
            return False
        model, opt = self.model, self.optimizer
        self.sync_free = True                                      # from here on the sample count stays on the device
        self._static = [t.detach().clone().contiguous() for t in (rays_o, rays_d, viewdirs, target)]
        opt.hyper_begin(model.density, model.k0)                  # creates the device-side step sizes; eager steps use them too
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                              # (torch: warm up on a side stream before capturing)
            for i in range(warmup):
                self._eager(*self._static, global_step + i)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        # the capture pass runs the Python of one step without executing its kernels: put the host-side state back after
        steps = {p: st['step'] for p, st in opt.state.items()}
        lrs = [g['lr'] for g in opt.param_groups]
        opt.hyper_begin(model.density, model.k0)
        graph = torch.cuda.CUDAGraph()
        self._capturing = True
        try:
            with torch.cuda.graph(graph):
                self._static_loss = self._eager(*self._static, global_step + warmup)
        finally:
            self._capturing = False
        for p, n in steps.items():
            opt.state[p]['step'] = n
        for g, lr in zip(opt.param_groups, lrs):
            g['lr'] = lr
        self._graph = graph
        return True

    def _replay(self, rays_o, rays_d, viewdirs, target):
        srcs = (rays_o, rays_d, viewdirs, target)
        if all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape == d.shape for t, d in zip(srcs, self._static)):
            n = len(srcs)                                   # the four inputs in one launch (csrc/loss.hip copy_multi)
            with L.device_of(rays_o):
                L.call('dvgo_copy_multi', (ctypes.c_void_p * n)(*[d.data_ptr() for d in self._static]),
                       (ctypes.c_void_p * n)(*[t.data_ptr() for t in srcs]), (ctypes.c_int64 * n)(*[t.numel() for t in srcs]),
                       n, L.stream_of(rays_o))
        else:
            for dst, src in zip(self._static, srcs):
                dst.copy_(src, non_blocking=True)
        self.optimizer.hyper_begin(self.model.density, self.model.k0, advance=True)    # this step's Adam step sizes
        self._graph.replay()
        self._decay_lr()
        return self._static_loss

    def __call__(self, rays_o, rays_d, viewdirs, target, global_step):
        """rays are this rank's shard; returns the (local share of the) loss as a 0-dim tensor (after `capture()`: a
        tensor that the next call overwrites)."""
        ray_grad = torch.is_grad_enabled() and (rays_o.requires_grad or rays_d.requires_grad)
        if ray_grad and self.world > 1:
            raise NotImplementedError('TrainStep: rays that require grad (learnable poses) are not built for data-parallel '
                                      'training: the pose gradient would need its own reduction')
        # (a captured graph holds copies of the rays: it cannot return a gradient to them.  Such a call runs eagerly)
        if self._graph is not None and rays_o.shape == self._static[0].shape and not ray_grad:
            return self._replay(rays_o, rays_d, viewdirs, target)
        return self._eager(rays_o, rays_d, viewdirs, target, global_step)

    def _tv_weighted(self):
        """Some regulariser of `_tv_add_grad` has a positive weight."""
        return bool(self.cfg['weight_tv_density'] > 0 or self.cfg['weight_tv_k0'] > 0 or self.plane_reg_on or self.density_reg_on)

    def _plan(self, rays_o, global_step):
        cfg, model, opt = self.cfg, self.model, self.optimizer
        tv = cfg['tv_after'] < global_step < cfg['tv_before'] and global_step % cfg['tv_every'] == 0 and self._tv_weighted()
        density, k0 = getattr(model, 'density', None), getattr(model, 'k0', None)
        # may the march's brick scatter apply the grid update itself?  One GPU: from its own tiles.  Data parallel: from the
        # all-reduced tiles of the bricks any rank touched (fused.brick_union) while that union stays small.
        own = (self.rows_adam and not tv and not self.k0_idle and not self.contracted and isinstance(opt, MaskedAdam)
               and isinstance(density, nn.Parameter) and isinstance(k0, nn.Parameter) and density.is_cuda)
        fuse_adam = own and opt.can_fuse_grid_step(density, k0)
        if self.dp is not None:                        # (dense gradients unless the tile path takes the step)
            path = 'tiles' if (fuse_adam and self.brick_sparse and getattr(model, 'fused', False)) else 'dense'
        else:
            path = 'fused' if fuse_adam else 'rows' if (own and opt.can_step_grid_rows(density, k0)) else 'dense'
        return _Plan(path, tv, bool(self.sync_free and self.fused_loss and rays_o.is_cuda
                                    and hasattr(model, 'can_keep_count_on_device') and model.can_keep_count_on_device()))

    def _decay_lr(self):
        for group in self.optimizer.param_groups:                                                  # run.py:401-406
            group['lr'] = group['lr'] * self.decay_factor

    def _eager(self, rays_o, rays_d, viewdirs, target, global_step):
        cfg, model, opt, dp = self.cfg, self.model, self.optimizer, self.dp
        if isinstance(opt, MaskedAdam) and opt.hyper_dev is not None and not self._capturing:
            opt.hyper_begin(model.density, model.k0)   # device-side step sizes of this step (see capture())
        plan = self._plan(rays_o, global_step)
        n_global = rays_o.shape[0] * self.world
        density, k0 = getattr(model, 'density', None), getattr(model, 'k0', None)
        extra = {'_capacity': True} if plan.keep_count else {}
        with (brick_union(dp.pg, dp.BRICK_SPARSE_MAX) if plan.path == 'tiles' else contextlib.nullcontext()) as bu:
            res = model(rays_o, rays_d, viewdirs, global_step=global_step, **self.render_kwargs, **extra)
            opt.zero_grad(set_to_none=True)
            loss_fn = fused_render_loss if (self.fused_loss and res['rgb_marched'].is_cuda) else render_loss
            loss = loss_fn(res, target, n_global, cfg)
            dist_loss = distortion_term(res, n_global, cfg) if loss_fn is fused_render_loss else None
            if dist_loss is not None:
                loss = loss + dist_loss
            if self.track_mse:
                self.last_mse = cfg['weight_main'] * (res['rgb_marched'].detach() - target).pow(2).sum() / (3 * n_global)
            # who updates the grids, now that the tile path knows (identical on every rank: decided from the all-reduced
            # brick counts); 'tiles' that stay: every rank is about to update the whole grid inside the backward
            path = 'dense' if (plan.path == 'tiles' and not bu.sparse) else plan.path
            if path == 'tiles':
                dp.whole_grid_update_ahead()
            self.last_fused_adam = path in ('fused', 'tiles')
            # backward order: ... colour-head data gradient -> grid scatters.  One GPU: the colour head's weight-gradient
            # kernel runs on a second stream beside the scatters.  Data parallel: it is postponed until the grid
            # all-reduce has been STARTED -- its persistent workgroups fill every CU, and RCCL's kernels, arriving
            # second, would sit behind them; arriving first they keep their CUs and the two overlap
            rows = (grid_rows_capture(density, k0, adam=(lambda: opt.grid_step_args(density, k0)) if self.last_fused_adam else None)
                    if path != 'dense' else contextlib.nullcontext())
            # the second stream pays on kernel-bound steps (the weight-gradient kernel beside the grid scatter: -0.3 ms at
            # 2 M samples) and costs on launch-bound ones (stream switches and event records on the host: +0.1 ms at 0.2 M)
            n_samples = self._sample_count(res)
            side = self.overlap_wgrad and dp is None and n_samples >= self.OVERLAP_MIN_SAMPLES
            with defer_wgrad(side_stream=side) as deferred, rows as cap:
                _FusedLoss.unit_grad = True
                try:
                    loss.backward()
                finally:
                    _FusedLoss.unit_grad = False
        # what the backward left: 'stepped' (both grids were updated inside it, csrc/brick.hip), gradient 'rows', or 'dense' .grad
        outcome = 'dense' if cap is None else 'stepped' if cap.stepped else 'rows' if cap.G is not None else 'dense'
        if outcome == 'stepped':
            assert density.grad is None and k0.grad is None
        elif outcome == 'rows':
            if density.grad is None and k0.grad is None:
                opt.step_grid_rows(density, k0, cap.G)            # (.grad of the two grids is None: step() below skips them)
            else:                                                 # more than one march in the graph: fold the rows back
                gd, gk = split_grid_rows(cap.G, density, k0)
                density.grad = gd if density.grad is None else density.grad + gd
                k0.grad = gk if k0.grad is None else k0.grad + gk
            cap.G = None
        if dp is None:
            deferred.flush()
            self.last_mode = 'single'
            if plan.tv:
                self._tv_add_grad(global_step, n_global)
            opt.step()
        else:
            # (tiles that said "dense": the all-reduced brick counts have settled it, no touched-voxel probe)
            dp.start(bu.bytes_on_wire if outcome == 'stepped' else None, probe=self.touched_reduce and bu is None)
            deferred.flush()
            slab = dp.wait()
            if plan.tv:
                self._tv_add_grad(global_step, n_global, **slab)
            gathers = dp.finish()
            opt.step()
            for wk in gathers:
                wk.wait()
            self.last_mode, self.last_wire_bytes = dp.last_mode, dp.last_wire_bytes
        self._decay_lr()
        return loss.detach()

    def _tv_add_grad(self, global_step, n_global, **x_range):
        """run.py:389-395, after the grid gradients have been reduced (data parallel: on the owned slab when sharded)."""
        cfg, dense = self.cfg, global_step < self.cfg['tv_dense_before']
        if cfg['weight_tv_density'] > 0:
            self.model.density_total_variation_add_grad(cfg['weight_tv_density'] / n_global, dense, **x_range)
        if cfg['weight_tv_k0'] > 0:
            self.model.k0_total_variation_add_grad(cfg['weight_tv_k0'] / n_global, dense, **x_range)
        if self.density_reg_on:                                  # colour planes and lines, then the density's: two launches
            self.model.plane_regularizers_add_grad(dense, **{k: w / n_global for k, w in {**self.plane_reg, **self.density_reg}.items()})
        elif self.plane_reg_on:                                  # planes and lines, one launch (one GPU: no slab)
            self.model.plane_regularizers_add_grad(dense, **{k: w / n_global for k, w in self.plane_reg.items()})
