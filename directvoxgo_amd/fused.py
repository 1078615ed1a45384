"""Fused ray march: the MI355X-native replacement of the op-by-op pipeline in
DirectVoxGO.forward (/root/reference/lib/dvgo.py:450-577).

Two autograd Functions wrap the kernels of csrc/march.hip:

  fused_march(...)   sampling + mask + density interp + activation + compositing weights +
                     both threshold filters + feature interp, returning exactly the tensors the
                     reference has after its 4th boolean compaction (lib/dvgo.py:488-509);
                     backward scatters into the density and feature grids.
  composite(...)     per-ray weighted colour sum + background (lib/dvgo.py:554-559), optional
                     depth (lib/dvgo.py:569-576).

One host sync per forward (the survivor count M3, needed to size the outputs); the reference
needs five.

  fused_march_vm(...)  `fused_march(..., positions=True)` for TensoRFVoxGO, whose density is a sum of plane
                     times line products and not a grid (csrc/march_vm.hip); the backward leaves one
                     gradient per record and hands the scatter to ops.vm_density_bwd.
  fused_march_contract(...)  the march of DirectContractedVoxGO over its table of sample distances in contracted space
                     (csrc/march_contract.hip): sampler, thinning, occupancy, density, alpha and weights in one launch;
                     the backward leaves one gradient per record and hands the scatter to dvgo_grid_sample_bwd.  With
                     `raygrad=True` it also returns the rays' gradient: the per-record gradients through the trilinear
                     position gradient and csrc/contract_raygrad.hip (camera-pose refinement of unbounded scenes).

`fused_march(..., positions=True, raygrad=True)` and `fused_march_vm(..., raygrad=True)` differentiate their rays as well
(csrc/march_raygrad.hip: dvgo_march_ray_bwd_pts, dvgo_march_vm_ray_bwd, one wavefront per ray over the march's own
records): the returned positions are differentiable, and the backward's first launch sums, per ray, the density's share
of every record and the gradient that arrived for the positions.  The defaults refuse such rays, as before.
"""
import math

import torch

from . import _lib as L
from ._lib import check_f32, check_input, f3, stream_of
from .ops import _grid_geom, _kernel_tensors, _plane_list, _vm_geom, _vm_grad_buffers, vm_density_bwd
from .shade import march_positions          # (shade.py imports nothing of this module: no cycle to break)

# scratch budget for fixed-stride records (16 B per potential sample)
_MAX_STRIDE_SCRATCH_BYTES = 4 << 30


class _MarchConstants:
    """What the config of every fused march holds: the bounds of the grids, the activation's constants and the occupancy mask
    with its scale / shift.  Model constants travel to the fused kernels as kernel arguments, so they are kept as host arrays;
    the device tensors serve the ops that take them from memory (the prepare kernel, dvgo_grid_sample_bwd)."""

    def __init__(self, xyz_min, xyz_max, act_shift, interval, fast_color_thres, mask, xyz2ijk_scale, xyz2ijk_shift):
        self.xyz_min_t, self.xyz_max_t = xyz_min, xyz_max
        self.xyz_min_h, self.xyz_max_h = f3(xyz_min), f3(xyz_max)
        self.act_shift = float(act_shift)
        self.interval = float(interval)
        self.thres = float(fast_color_thres)
        self.mask = mask
        self.scale_h = f3(xyz2ijk_scale) if mask is not None else f3([0, 0, 0])
        self.shift_h = f3(xyz2ijk_shift) if mask is not None else f3([0, 0, 0])


class MarchConfig(_MarchConstants):
    """Host-side constants of one model/render setting."""

    def __init__(self, xyz_min, xyz_max, stepdist, act_shift, interval, fast_color_thres, near, far,
                 mask=None, xyz2ijk_scale=None, xyz2ijk_shift=None, ndc_samples=0):
        super().__init__(xyz_min, xyz_max, act_shift, interval, fast_color_thres, mask, xyz2ijk_scale, xyz2ijk_shift)
        self.stepdist = float(stepdist)
        self.near, self.far = float(near), float(far)
        # > 0: forward-facing / MPI sampling (lib/dmpigo.py:173-198): every ray has exactly ndc_samples
        # samples at o + d * s/(ndc_samples-1); encoded for the kernels as stepdist = -(ndc_samples-1)
        self.ndc_samples = int(ndc_samples)
        if self.ndc_samples > 0:
            self.stepdist = -float(self.ndc_samples - 1)


def _rec_stride(cfg, n_rays):
    """Upper bound of N_steps: t_min,t_max are clamped to [near,far] (render_utils_kernel.cu:32-33)
    so N_steps <= ceil((far-near)/stepdist) (+1 for the division rounding)."""
    span = (cfg.far - cfg.near) / cfg.stepdist
    if not math.isfinite(span) or span < 0:
        return 0
    stride = int(math.ceil(span)) + 2
    if stride * n_rays * 16 > _MAX_STRIDE_SCRATCH_BYTES:
        return 0
    return stride


# Owner-computes gradient scatter (csrc/brick.hip): samples are listed per 8x8x8 brick, one workgroup sums a brick;
# no float atomics, no zero-fill.  The default whenever both grids want a gradient, share the lattice and the
# feature grid is channels-last with a built channel count; the atomic scatters below remain as A/B variants.
# The scans between march_density and march_gather (per-ray offsets, brick tables) done by march_density's last workgroup
# instead of a launch of their own (False: dvgo_march_scans, A/B and tests)
TAIL_SCANS = False        # (with 256-thread workgroups the tail is 8 serial passes: +30 us; pays with the 16-ray kernel)
_TICKETS = {}


def _tail_ticket(dev, st):
    """The ticket word of the tail: one zeroed int32 per (device, stream); the kernel leaves it at zero."""
    key = (dev.index, int(st.value or 0))
    t = _TICKETS.get(key)
    if t is None:
        t = _TICKETS[key] = torch.zeros(1, dtype=torch.int32, device=dev)
    return t


BRICK_SLICE = None          # entries per work item of the brick kernel (None: the library's default)
BRICK_SCATTER = True
BRICK_CHANNELS = (3, 4, 9, 12)

# A/B switch (tests, tools): scatter both grid gradients through one buffer of 64-byte voxel rows
COMBINED_GRID_GRAD = True
COMBINED_MIN_RATIO = 6          # use it when kept samples * ratio >= voxels (tests set 1e9 to force it)


class grid_rows_capture:
    """Context manager for a training step that owns the optimizer: inside it the march backward does NOT produce
    `k0.grad` / `density.grad` (those two stay `None`).  Either
      * `adam` is given (a callable returning the Adam argument group of dvgo_brick_accumulate, see
        `MaskedAdam.grid_step_args`) and the brick scatter applies the masked Adam update of both grids in place, from
        the brick's gradient tile in LDS -- the gradient never exists in memory (`.stepped` is set); or
      * the atomic scatter into combined gradient rows hands them over (`.G`: [n_vox, 16] = 12 feature channels, the
        density gradient, pad) so that the optimizer can update both grids straight from the rows
        (`MaskedAdam.step_grid_rows`).
    Only for the (density, k0) parameters given."""
    _active = None

    def __init__(self, density, k0, adam=None):
        self.density, self.k0, self.G, self.adam, self.stepped = density, k0, None, adam, False

    def __enter__(self):
        self.G, self.stepped = None, False
        grid_rows_capture._active = self
        return self

    def __exit__(self, *exc):
        grid_rows_capture._active = None
        return False


class brick_union:
    """Context manager of a data-parallel training step (train.TrainStep, world > 1): the march's brick scatter then moves
    the grid gradient between the ranks as whole brick tiles.
      forward : the per-brick counts of every rank are summed (one 4 * n_bricks byte all-reduce, started right after
                march_density and waited for behind the local scans), `dvgo_brick_scan` turns the sum into the list of the
                bricks ANY rank touched, and its length rides on the forward's one host read;
      backward: every rank writes one 512 x 16 tile per listed brick (zeros where it has no sample), ONE all-reduce sums the
                compact tile buffer, and every rank applies the same masked Adam update from the summed tiles
                (grid_rows_capture.adam) -- parameters and moments stay replicated, no dense gradient, no host-side index.
    `.sparse` (after the forward): True when the tile path takes the step -- the union is at most `max_frac` of the bricks;
    otherwise the backward produces dense gradients for the reduce-scatter path.  Rank-invariant by construction (it is
    decided from the all-reduced counts)."""
    _active = None

    def __init__(self, group=None, max_frac=0.5):
        self.group, self.max_frac = group, max_frac
        self.sparse, self.n_union, self.n_bricks, self.bytes_on_wire = None, 0, 0, 0

    def __enter__(self):
        brick_union._active = self
        return self

    def __exit__(self, *exc):
        brick_union._active = None
        return False


def split_grid_rows(G, density, k0):
    """Combined gradient rows -> (density.grad, k0.grad) in the parameters' own layouts."""
    gk = torch.empty_like(k0, memory_format=torch.preserve_format)
    gd = torch.empty_like(density)
    with L.device_of(G):
        L.call('dvgo_grid_grad_split', G, density.numel(), 16, k0.shape[1], gk, gd, stream_of(G))
    return gd, gk


class _BrickPlan:
    """The brick tables of one forward (csrc/brick.hip), from the counting in march_density to the backward that consumes
    them; `ctx.plan` of _FusedMarch.  `n_bricks == 0`: no brick scatter for this forward, every table is None.
      counts [n_bricks] samples per brick; offsets [n_bricks + 1] list offsets (offsets[-1]: the list total);
      cursor [n_bricks] fill cursors of march_density_bwd (consumed: one backward per forward);
      heavy bricks, else None and slice_len == n_extra_max == 0: extra_off [n_bricks + 1] extra work items, active
      [n_bricks + 1] the non-empty bricks, extra_brick [n_extra_max] the brick of each extra item, arrive = `counts`,
      which the scan clears into the slices' arrival counters.
    n_entries: the list total (or its bound) once the forward has learnt it."""

    def __init__(self, want_grads, density, k0, n_rays, cap):
        C, X, Y, Z, sC, sX, sY, sZ = _grid_geom(k0)
        self.n_bricks = self.slice_len = self.n_extra_max = self.n_entries = 0
        self.counts = self.offsets = self.cursor = self.extra_off = self.active = self.extra_brick = self.arrive = None
        # training: count, per 8^3 brick, the samples the backward will list for it
        if not (BRICK_SCATTER and want_grads[0] and want_grads[1] and C in BRICK_CHANNELS
                and tuple(density.shape[2:]) == (X, Y, Z) and (sC, sZ, sY, sX) == (1, C, Z * C, Y * Z * C)
                and k0.data_ptr() % 16 == 0 and n_rays > 0 and 8 * cap < 1 << 31):       # int32 list offsets
            return
        dev = density.device
        nb = self.n_bricks = L.lib().dvgo_n_bricks(X, Y, Z)
        self.counts = torch.zeros(nb, dtype=torch.int32, device=dev)
        tabs = torch.empty((3, nb + 1), dtype=torch.int32, device=dev)    # list offsets, extra items, non-empty bricks
        self.offsets = tabs[0]
        self.cursor = torch.empty(nb, dtype=torch.int32, device=dev)
        # heavy bricks: extra work items <= entries / slice, entries <= 8 per record slot.  The packed scan of
        # csrc/scan.h has 28 bits for entries and 18 each for extra items and non-empty bricks: beyond that
        # (render-sized batches, 512^3 grids) every brick runs as one workgroup
        sl = BRICK_SLICE or L.lib().dvgo_brick_slice()
        if 8 * cap < 1 << 28 and nb < 1 << 18 and 8 * max(cap, 1) // sl < 1 << 18:
            self.slice_len = sl
            self.n_extra_max = 8 * max(cap, 1) // sl
            self.extra_off, self.active, self.arrive = tabs[1], tabs[2], self.counts
            self.extra_brick = torch.empty(max(self.n_extra_max, 1), dtype=torch.int32, device=dev)


def _scans(plan, n3, N, off3, tail, union, list_total, st):
    """Every scan between march_density and march_gather: n3 -> off3 (per-ray offsets), the plan's counts -> its tables and,
    data parallel (`union` = the all-reduce of the counts, in flight), the union's counts -> the table of the bricks any
    rank touched, which is returned.  `list_total`: the host is about to read off3[N + 1], the plan's list total."""
    nb = plan.n_bricks
    if tail:
        pass                        # the last workgroup of march_density has written off3 and the brick tables
    elif N <= 16384:                # both scans in one launch (one workgroup each)
        L.call('dvgo_march_scans', n3, N, off3, plan.counts, nb, plan.offsets, plan.cursor, plan.extra_off, plan.active,
               plan.extra_brick, plan.n_extra_max, plan.slice_len, st)
    else:                           # render-sized batches: the multi-workgroup scan
        L.call('dvgo_exclusive_scan_i32', n3, N, off3, st)
        if nb:
            L.call('dvgo_brick_scan', plan.counts, nb, plan.offsets, plan.cursor, plan.extra_off, plan.active,
                   plan.extra_brick, plan.n_extra_max, plan.slice_len, st)
    union_active = None
    if union is not None:
        union_cnt, work = union
        work.wait()
        tabs = torch.empty((4, nb + 1), dtype=torch.int32, device=n3.device)     # off, cursor, extra, active
        L.call('dvgo_brick_scan', union_cnt, nb, tabs[0], tabs[1], tabs[2], tabs[3], tabs[1], 0, 1 << 30, st)
        union_active = tabs[3]
    if list_total and nb and N > 16384:         # (the multi-workgroup scan path does not write the list total)
        off3[N + 1] = plan.offsets[-1]
    return union_active


# the Adam group of dvgo_brick_accumulate (p_k0 .. step_sizes_dev) when the launch applies no update
_NO_ADAM = (None, None, None, 0.0, 0, None, None, None, 0.0, 0, 0.0, 0.0, 0.0, None)


class _FusedMarch(torch.autograd.Function):
    @staticmethod
    def forward(ctx, density, k0, rays_o, rays_d, cfg, capacity=False, positions=False, raygrad=False):
        for x, n in ((rays_o, 'rays_o'), (rays_d, 'rays_d')):
            check_input(x, n); check_f32(x, n)
        if not (density.is_cuda and k0.is_cuda):
            raise RuntimeError('density must be a CUDA tensor')
        check_f32(density, 'density'); check_f32(k0, 'k0')
        if not density.is_contiguous():
            raise RuntimeError('density must be contiguous')
        dev = rays_o.device
        N = rays_o.shape[0]
        _, X, Y, Z, _, _, _, _ = _grid_geom(density)
        C, kX, kY, kZ, sC, sX, sY, sZ = _grid_geom(k0)
        assert (kX, kY, kZ) == (X, Y, Z), 'density and k0 must share world_size'
        st = stream_of(rays_o)
        ndc = cfg.ndc_samples > 0
        # rays that require grad (camera-pose refinement): the backward also launches dvgo_march_ray_bwd (fused_march has
        # refused what that kernel does not differentiate)
        ray_grad = bool(ctx.needs_input_grad[2] or ctx.needs_input_grad[3]) and not (positions or ndc)
        # ... and with positions (raygrad=True): dvgo_march_ray_bwd_pts, which takes the gradient that arrives for the
        # returned positions in place of the k0 term
        pts_grad = bool(ctx.needs_input_grad[2] or ctx.needs_input_grad[3]) and bool(positions and raygrad) and not ndc
        stride = cfg.ndc_samples if ndc else _rec_stride(cfg, N)

        setup_in_march = (not ndc) and stride > 0        # K1-K3 inside march_density: one launch less
        if ndc:
            n_steps = torch.full((N,), cfg.ndc_samples, dtype=torch.int64, device=dev)
            start, dirs = rays_o, rays_d
        else:
            n_steps = torch.empty(N, dtype=torch.int64, device=dev)
            start = torch.empty((N, 3), dtype=torch.float32, device=dev)
            dirs = torch.empty((N, 3), dtype=torch.float32, device=dev)
        cum = torch.empty(N, dtype=torch.int64, device=dev) if stride == 0 else None
        n2 = torch.empty(N, dtype=torch.int32, device=dev)
        n3 = torch.empty(N, dtype=torch.int32, device=dev)
        last = torch.empty(N, dtype=torch.float32, device=dev)
        off3 = torch.empty(N + 2, dtype=torch.int64, device=dev)     # [N]: surviving samples, [N + 1]: brick-list entries
        with L.device_of(rays_o):
            if not ndc and not setup_in_march:
                t_min = torch.empty(N, dtype=torch.float32, device=dev)
                t_max = torch.empty_like(t_min)
                L.call('dvgo_sample_pts_prepare', rays_o, rays_d, cfg.xyz_min_t, cfg.xyz_max_t, cfg.near, cfg.far,
                       cfg.stepdist, N, t_min, t_max, n_steps, cum, start, dirs, st)
            if stride == 0:
                cap = int(cum[-1].item()) if N > 0 else 0     # exact layout: one extra host read
            else:
                cap = stride * N
            rec2 = torch.empty((max(cap, 1), 4), dtype=torch.float32, device=dev)
            plan = _BrickPlan(ctx.needs_input_grad, density, k0, N, cap)
            mask = cfg.mask
            mshape = mask.shape if mask is not None else (0, 0, 0)
            tail = TAIL_SCANS and 0 < N <= 16384          # the scans ride on march_density's last workgroup
            L.call('dvgo_march_density', start, dirs, n_steps, cum, stride, N, cfg.xyz_min_h, cfg.xyz_max_h, cfg.stepdist,
                   mask, mshape[0], mshape[1], mshape[2], cfg.scale_h, cfg.shift_h, density, X, Y, Z, cfg.act_shift,
                   cfg.interval, cfg.thres, rec2, n2, n3, last, plan.counts, rays_o if setup_in_march else None,
                   rays_d if setup_in_march else None, cfg.near, cfg.far, _tail_ticket(dev, st) if tail else None, off3,
                   plan.n_bricks, plan.offsets, plan.cursor, plan.extra_off, plan.active, plan.extra_brick,
                   plan.n_extra_max, plan.slice_len, st)
            bu = brick_union._active if (plan.extra_brick is not None and ctx.needs_input_grad[0]) else None
            union = None
            if bu is not None:
                import torch.distributed as dist
                union_cnt = plan.counts.clone()                     # (the local scan below clears the counters)
                union = (union_cnt, dist.all_reduce(union_cnt, op=dist.ReduceOp.SUM, group=bu.group, async_op=True))
            # training step (train.py): the surviving-sample count stays on the device.  The outputs are sized by
            # their upper bound -- every step of every ray -- and every consumer is handed off3[N] as a device
            # pointer (`m_dev`): no host synchronisation in the forward at all.  Rows past the count are garbage.
            padded = bool(capacity and stride > 0 and plan.n_bricks)
            union_active = _scans(plan, n3, N, off3, tail, union, not padded, st)
            if padded:
                M3 = stride * N
                plan.n_entries = 8 * M3                         # a sample touches at most 2 x 2 x 2 bricks
            elif bu is not None:                                # (data parallel: the union size rides along)
                M3, plan.n_entries, n_union = torch.cat((off3, union_active[-1:].long()))[N:N + 3].tolist()
                bu.n_union, bu.n_bricks, bu.sparse = n_union, plan.n_bricks, n_union <= bu.max_frac * plan.n_bricks
            elif plan.n_bricks:
                M3, plan.n_entries = off3[N:N + 2].tolist()     # the one host sync: 16 contiguous bytes, no gather launch
            else:
                M3 = int(off3[N].item())                       # the one host sync of the fused forward
            ray_id = torch.empty(M3, dtype=torch.int64, device=dev)
            step_id = torch.empty(M3, dtype=torch.int64, device=dev)
            weights = torch.empty(M3, dtype=torch.float32, device=dev)
            alpha = torch.empty(M3, dtype=torch.float32, device=dev)
            feat = torch.empty((M3, C), dtype=torch.float32, device=dev)
            L.call('dvgo_march_gather', rec2, n2, n_steps, cum, stride, off3, N, M3, start, dirs, cfg.stepdist, cfg.xyz_min_h,
                   cfg.xyz_max_h, k0, C, X, Y, Z, sC, sX, sY, sZ, ray_id, step_id, weights, alpha, feat, st)
            if positions:              # the kept samples' positions in place of the (zero-channel) features
                feat = march_positions(start, dirs, ray_id, step_id, cfg.stepdist)
        ctx.cfg = cfg
        ctx.geom = (X, Y, Z, C, sC, sX, sY, sZ, stride, N)
        ctx.plan = plan if plan.n_bricks else None
        ctx.union = (bu, union_active, bu.n_union) if (bu is not None and bu.sparse) else None
        ctx.padded = padded
        ctx.density_meta, ctx.k0_meta = density, k0
        ctx.ray_grad, ctx.pts_grad = ray_grad, pts_grad
        ctx.save_for_backward(rec2, n2, n_steps, cum if cum is not None else n_steps, off3, start, dirs, last,
                              ray_id, step_id, *((rays_o, rays_d) if (ray_grad or pts_grad) else ()))
        off3 = off3[:N + 1]
        ctx.mark_non_differentiable(alpha, ray_id, step_id, off3, *((feat,) if (positions and not pts_grad) else ()))
        ctx.set_materialize_grads(False)     # no zero-filled [M3] int64 'gradients' for the id outputs (33 MB per step)
        return weights, alpha, last, feat, ray_id, step_id, off3

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_w, _g_alpha, g_last, g_feat, _g_rid, _g_sid, _g_off):
        rec2, n2, n_steps, cum, off3, start, dirs, last, ray_id, step_id = ctx.saved_tensors[:10]
        X, Y, Z, C, sC, sX, sY, sZ, stride, N = ctx.geom
        cfg = ctx.cfg
        M3 = ray_id.shape[0]
        st = stream_of(start)
        grad_density = grad_k0 = None
        dev = start.device
        with L.device_of(start):
            want_k0 = ctx.needs_input_grad[1] and g_feat is not None and C > 0
            want_d = ctx.needs_input_grad[0]
            gw = gl = None
            if want_d or ctx.ray_grad or ctx.pts_grad:
                gw = g_w.contiguous() if g_w is not None else torch.zeros(M3, dtype=torch.float32, device=dev)
                gl = g_last.contiguous() if g_last is not None else None
            rays = (None, None)
            if ctx.ray_grad or ctx.pts_grad:
                # FIRST, before any other launch of this backward: the brick scatter below may apply the optimizer's
                # update to both grids in place (grid_rows_capture.adam), and this kernel must read the grids the
                # forward read.  Same stream, so launch order is execution order.
                rays_o, rays_d = ctx.saved_tensors[10:]
                go = torch.empty((N, 3), dtype=torch.float32, device=dev)
                gd = torch.empty((N, 3), dtype=torch.float32, device=dev)
                if ctx.ray_grad:       # the k0 grid and the gradient of its features
                    entry, colour, g_rows = 'dvgo_march_ray_bwd', (ctx.k0_meta, C, sC, sX, sY, sZ), g_feat if C > 0 else None
                else:                  # `g_feat` is the gradient that arrived for the positions (None: none did)
                    entry, colour, g_rows = 'dvgo_march_ray_bwd_pts', (), g_feat
                L.call(entry, rec2, n2, n_steps, cum if stride == 0 else None, stride, off3, N, start, dirs,
                       cfg.stepdist, cfg.xyz_min_h, cfg.xyz_max_h, last, cfg.interval, rays_o, rays_d, cfg.near, cfg.far,
                       ctx.density_meta, X, Y, Z, *colour, gw, gl, g_rows.contiguous() if g_rows is not None else None, go, gd, st)
                rays = (go if ctx.needs_input_grad[2] else None, gd if ctx.needs_input_grad[3] else None)

            def density_bwd(dst, dst_stride, kept, cursor=None, recs=None):
                L.call('dvgo_march_density_bwd', rec2, n2, n_steps, cum if stride == 0 else None, stride, off3, N, start, dirs,
                       cfg.stepdist, cfg.xyz_min_h, cfg.xyz_max_h, last, cfg.interval, gw, gl, X, Y, Z, dst, dst_stride, kept,
                       cursor, recs, st)

            plan = ctx.plan if (want_k0 and want_d and BRICK_SCATTER) else None
            if ctx.padded and plan is None:
                raise RuntimeError('capacity-mode forward (device-side sample count) needs the brick scatter backward for both grids')
            if plan is not None:
                ctx.plan = None                                 # the fill cursors are consumed: one backward per forward
                return _brick_backward(ctx, plan, density_bwd, g_feat, start, dirs, st) + rays + (None,) * 4

            # worth its two extra full-grid passes (zero 64 B, split 116 B per voxel) from ~1 kept sample per 6 voxels
            combined = (COMBINED_GRID_GRAD and want_k0 and want_d and C == 12 and M3 * COMBINED_MIN_RATIO >= X * Y * Z and tuple(ctx.density_meta.shape[2:]) == (X, Y, Z)
                        and (sC, sZ, sY, sX) == (1, C, Z * C, Y * Z * C))
            if combined:
                # both grids share the voxel lattice: one scatter into 64-byte rows (12 feature channels + the
                # density gradient), then a streaming split into the two dense gradients
                G = torch.zeros((X * Y * Z, 16), dtype=torch.float32, device=dev)
                kept = torch.empty(M3, dtype=torch.float32, device=dev)
                density_bwd(G[:, 12:], 16, kept)
                L.call('dvgo_march_feat_bwd', g_feat.contiguous(), kept, ray_id, step_id, M3, start, dirs, cfg.stepdist,
                       cfg.xyz_min_h, cfg.xyz_max_h, C, X, Y, Z, 1, Y * Z * 16, Z * 16, 16, G, st)
                cap = grid_rows_capture._active
                if cap is not None and cap.G is None and cap.density is ctx.density_meta and cap.k0 is ctx.k0_meta:
                    cap.G = G                  # the optimizer consumes the rows; no dense gradients are produced
                    return (None, None) + rays + (None,) * 4
                grad_k0 = torch.empty_like(ctx.k0_meta, memory_format=torch.preserve_format)
                grad_density = torch.empty_like(ctx.density_meta)
                assert grad_k0.stride() == ctx.k0_meta.stride() and grad_density.is_contiguous()
                L.call('dvgo_grid_grad_split', G, X * Y * Z, 16, C, grad_k0, grad_density, st)
            else:
                if want_k0:
                    grad_k0 = torch.zeros_like(ctx.k0_meta, memory_format=torch.preserve_format)
                    assert grad_k0.stride() == ctx.k0_meta.stride()
                    L.call('dvgo_march_feat_bwd', g_feat.contiguous(), None, ray_id, step_id, M3, start, dirs, cfg.stepdist,
                           cfg.xyz_min_h, cfg.xyz_max_h, C, X, Y, Z, sC, sX, sY, sZ, grad_k0, st)
                if want_d:
                    grad_density = torch.zeros_like(ctx.density_meta)
                    density_bwd(grad_density, 1, None)
        return (grad_density, grad_k0) + rays + (None,) * 4


def _brick_backward(ctx, plan, density_bwd, g_feat, start, dirs, st):
    """Owner-computes scatter: list every sample per brick, then one workgroup sums each brick.  -> (density.grad, k0.grad),
    both None when the scatter applied the optimizer's update itself (grid_rows_capture.adam)."""
    X, Y, Z, C = ctx.geom[:4]
    dev = start.device
    recs = torch.empty((max(plan.n_entries, 1), 4), dtype=torch.int32, device=dev)
    density_bwd(None, 1, None, plan.cursor, recs)
    lists = (recs, start, dirs, g_feat.contiguous())
    scratch, n_extra, cfg = None, 0, ctx.cfg
    if plan.extra_brick is not None:        # heavy bricks run as several work items (slices of the list) that meet in scratch tiles
        n_extra = min(plan.extra_brick.shape[0], plan.n_entries // plan.slice_len)
        scratch = torch.empty((2 * n_extra + 1, 512 * ((C + 4) // 4 * 4)), dtype=torch.float32, device=dev)

    def accumulate(lists, active=None, grad_k0=None, grad_density=None, adam=_NO_ADAM, tiles=None, mode=0):
        """The one issuer of dvgo_brick_accumulate; the four modes are the calls below.  `lists`: None when the launch
        reads tiles instead; `active`: the union's brick table in place of the plan's own; `adam`: grid_step_args."""
        assert len(adam) == len(_NO_ADAM)
        recs, start, dirs, g_feat = lists or (None, None, None, None)
        L.call('dvgo_brick_accumulate', plan.offsets, plan.extra_off, active if active is not None else plan.active,
               plan.extra_brick, plan.arrive, scratch, n_extra, plan.slice_len, recs, start, dirs, cfg.stepdist, cfg.xyz_min_h,
               cfg.xyz_max_h, g_feat, C, X, Y, Z, grad_k0, grad_density, *adam, tiles, mode, st)

    cap = grid_rows_capture._active
    fuse = (cap is not None and cap.adam is not None and not cap.stepped and cap.density is ctx.density_meta
            and cap.k0 is ctx.k0_meta)
    if fuse and ctx.union is not None:
        # data parallel, sparse scene: tiles of the bricks any rank touched -> one all-reduce -> the same masked
        # Adam update from the summed tiles on every rank
        import torch.distributed as dist
        bu, union_active, n_union = ctx.union
        TS = (C + 4) // 4 * 4
        tiles = torch.empty((max(n_union, 1), 512 * TS), dtype=torch.float32, device=dev)
        accumulate(lists, active=union_active, tiles=tiles, mode=2)
        if n_union > 0:
            dist.all_reduce(tiles[:n_union], op=dist.ReduceOp.SUM, group=bu.group)
        bu.bytes_on_wire = n_union * 512 * TS * 4
        accumulate(None, active=union_active, adam=cap.adam(), tiles=tiles, mode=3)
    elif fuse and brick_union._active is None:
        accumulate(lists, adam=cap.adam())
    else:
        grad_k0 = torch.empty_like(ctx.k0_meta, memory_format=torch.preserve_format)
        grad_density = torch.empty_like(ctx.density_meta)
        assert grad_k0.stride() == ctx.k0_meta.stride() and grad_density.is_contiguous()
        accumulate(lists, grad_k0=grad_k0, grad_density=grad_density)
        return grad_density, grad_k0
    cap.stepped = True
    return None, None


@torch.no_grad()
def fused_hit(rays_o, rays_d, cfg):
    """bool [N]: rays with at least one in-box sample in occupied space (lib/dvgo.py:412-423), no sample
    list materialised."""
    rays_o, rays_d = rays_o.contiguous(), rays_d.contiguous()
    for x, n in ((rays_o, 'rays_o'), (rays_d, 'rays_d')):
        check_input(x, n); check_f32(x, n)
    N, dev = rays_o.shape[0], rays_o.device
    t_min = torch.empty(N, dtype=torch.float32, device=dev)
    t_max = torch.empty_like(t_min)
    n_steps = torch.empty(N, dtype=torch.int64, device=dev)
    start = torch.empty((N, 3), dtype=torch.float32, device=dev)
    dirs = torch.empty((N, 3), dtype=torch.float32, device=dev)
    hit = torch.empty(N, dtype=torch.bool, device=dev)
    mask = cfg.mask
    with L.device_of(rays_o):
        st = stream_of(rays_o)
        L.call('dvgo_sample_pts_prepare', rays_o, rays_d, cfg.xyz_min_t, cfg.xyz_max_t, cfg.near, cfg.far, cfg.stepdist, N,
               t_min, t_max, n_steps, None, start, dirs, st)
        L.call('dvgo_march_hit', start, dirs, n_steps, N, cfg.xyz_min_h, cfg.xyz_max_h, cfg.stepdist, mask, mask.shape[0],
               mask.shape[1], mask.shape[2], cfg.scale_h, cfg.shift_h, hit, st)
    return hit


def fused_march(density, k0, rays_o, rays_d, cfg, capacity=False, positions=False, raygrad=False):
    """-> weights [M3], raw_alpha [M3], alphainv_last [N], k0 features [M3,C], ray_id, step_id [M3],
    off3 [N+1] (exclusive offsets of each ray's samples in the M3 arrays).
    `capacity=True`: no host synchronisation; the M3-sized outputs are allocated at their upper bound and only their
    first off3[N] rows are defined (pass `off3[N:]` as `m_dev` to the consumers).
    `positions=True` (positional-encoding colour head): k0 must have zero channels (nothing is read from it) and the
    fourth output is the kept samples' positions [M3,3] instead of the features, with no gradient.
    `rays_o` / `rays_d` that require grad get one (csrc/march_raygrad.hip: march_ray_bwd, launched first in the backward; the
    stop-gradients are DirectVoxGO._forward_raygrad's); with `positions=True` or NDC sampling that is a NotImplementedError.
    `positions=True, raygrad=True` (HashVoxGO, VMTriPlaneVoxGO with raygrad='fused'): the same launches and the same bits, the
    returned positions are differentiable, and the backward launches dvgo_march_ray_bwd_pts first (csrc/march_raygrad.hip:
    the density's share per record plus the gradient that arrived for the positions, summed per ray with the same
    stop-gradients).  NDC sampling stays refused."""
    if torch.is_grad_enabled() and (rays_o.requires_grad or rays_d.requires_grad) and (
            (positions and not raygrad) or cfg.ndc_samples > 0):
        raise NotImplementedError('fused_march: rays that require grad are not differentiated through '
                                  + ('the positional-encoding head\'s position input' if (positions and not raygrad)
                                     else 'NDC sampling'))
    return _FusedMarch.apply(density, k0, rays_o.contiguous(), rays_d.contiguous(), cfg, capacity, positions, bool(raygrad))


def _records_to_samples(rec2, n2, n3, off3, off2, N, stride, cfg, st, start, dirs, stepdist, n_steps=None):
    """The forward tail of the record-per-gradient marches (_FusedMarchVM, _FusedMarchContract): the per-ray counts become
    offsets (n3 -> off3, n2 -> off2), ONE host read brings both totals -- M3 (kept samples, sizes the outputs) and M2
    (records, sizes the backward's per-record gradient) -- and dvgo_march_gather compacts the kept records into
    ray_id / step_id / weights / alpha.  -> M3, M2, ray_id, step_id, weights, alpha.
    The gather runs with no feature grid: zero channels of a 1 x 1 x 1 lattice.  In that mode it forms a uniform-step
    position from `start`, `dirs` and `stepdist` and uses it for nothing, so a march whose steps are not uniform passes any
    [N,3] floats for the first two (its rays_o / rays_d), and with a fixed stride it never reads `n_steps`: left out,
    off3 stands in (any non-null int64 pointer)."""
    dev = rec2.device
    L.call('dvgo_exclusive_scan_i32', n3, N, off3, st)
    torch.cumsum(n2, 0, dtype=torch.int64, out=off2[1:])
    M3, M2 = torch.stack((off3[N], off2[N])).tolist()          # the one host read: both counts
    ray_id = torch.empty(M3, dtype=torch.int64, device=dev)
    step_id = torch.empty(M3, dtype=torch.int64, device=dev)
    weights = torch.empty(M3, dtype=torch.float32, device=dev)
    alpha = torch.empty(M3, dtype=torch.float32, device=dev)
    L.call('dvgo_march_gather', rec2, n2, n_steps if n_steps is not None else off3, None, stride, off3, N, M3, start, dirs,
           stepdist, cfg.xyz_min_h, cfg.xyz_max_h, None, 0, 1, 1, 1, 1, 1, 1, 1, ray_id, step_id, weights, alpha, None, st)
    return M3, M2, ray_id, step_id, weights, alpha


def _record_grads(g_w, g_last, M3, M2, dev):
    """The backward preamble of the same marches -> gw [M3] (zeros when `weights` took no gradient), gl [N] or None, and
    the two per-record outputs of the walk, uninitialised: g_raw [M2] and the positions [M2, 3]."""
    gw = g_w.contiguous() if g_w is not None else torch.zeros(M3, dtype=torch.float32, device=dev)
    gl = g_last.contiguous() if g_last is not None else None
    return gw, gl, torch.empty(M2, dtype=torch.float32, device=dev), torch.empty((M2, 3), dtype=torch.float32, device=dev)


class _FusedMarchVM(torch.autograd.Function):
    """csrc/march_vm.hip: the march over TensoRFVoxGO's decomposed density.  Two host-visible counts, read together: M3
    (kept samples, sizes the outputs) and M2 (records, sizes the backward's per-record gradient)."""

    @staticmethod
    def forward(ctx, rays_o, rays_d, cfg, stride, raygrad, *tensors):
        for x, n in ((rays_o, 'rays_o'), (rays_d, 'rays_d')):
            check_input(x, n); check_f32(x, n)
        dev = rays_o.device
        N = rays_o.shape[0]
        cap = stride * N
        kt = _kernel_tensors(ctx, list(tensors), cap)        # the rule looks at the three planes; cap: the steps a launch may take
        g, R = _vm_geom(kt)
        st = stream_of(rays_o)
        n_steps = torch.empty(N, dtype=torch.int64, device=dev)
        start = torch.empty((N, 3), dtype=torch.float32, device=dev)
        dirs = torch.empty((N, 3), dtype=torch.float32, device=dev)
        n2 = torch.empty(N, dtype=torch.int32, device=dev)
        n3 = torch.empty(N, dtype=torch.int32, device=dev)
        last = torch.empty(N, dtype=torch.float32, device=dev)
        off3 = torch.empty(N + 1, dtype=torch.int64, device=dev)
        off2 = torch.zeros(N + 1, dtype=torch.int64, device=dev)
        rec2 = torch.empty((max(cap, 1), 4), dtype=torch.float32, device=dev)
        mask = cfg.mask
        mshape = mask.shape if mask is not None else (0, 0, 0)
        with L.device_of(rays_o):
            L.call('dvgo_march_vm_density', start, dirs, n_steps, stride, N, cfg.xyz_min_h, cfg.xyz_max_h, cfg.stepdist, mask,
                   mshape[0], mshape[1], mshape[2], cfg.scale_h, cfg.shift_h, *g, R, cfg.act_shift, cfg.interval, cfg.thres,
                   rec2, n2, n3, last, rays_o, rays_d, cfg.near, cfg.far, st)
            M3, M2, ray_id, step_id, weights, alpha = _records_to_samples(rec2, n2, n3, off3, off2, N, stride, cfg, st, start,
                                                                          dirs, cfg.stepdist, n_steps=n_steps)
            pts = march_positions(start, dirs, ray_id, step_id, cfg.stepdist)
        ctx.cfg, ctx.counts = cfg, (stride, N, M2, M3)
        # rays that require grad (raygrad=True): the backward launches dvgo_march_vm_ray_bwd first, and the positions
        # carry a gradient back to it
        ctx.ray_grad = bool(raygrad) and bool(ctx.needs_input_grad[0] or ctx.needs_input_grad[1])
        ctx.save_for_backward(rec2, n2, n_steps, off3, off2, start, dirs, last, *kt, *((rays_o, rays_d) if ctx.ray_grad else ()))
        ctx.mark_non_differentiable(alpha, ray_id, step_id, off3, *(() if ctx.ray_grad else (pts,)))
        ctx.set_materialize_grads(False)
        return weights, alpha, last, pts, ray_id, step_id, off3

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_w, _g_alpha, g_last, g_pts, _g_rid, _g_sid, _g_off):
        rec2, n2, n_steps, off3, off2, start, dirs, last, *kt = ctx.saved_tensors[:14]
        stride, N, M2, M3 = ctx.counts
        cfg = ctx.cfg
        needs = ctx.needs_input_grad[5:]
        if not any(needs) and not ctx.ray_grad:
            return (None,) * 11
        dev = start.device
        go = gd = None
        if ctx.ray_grad:
            # FIRST (the rule of _FusedMarch.backward), and also when the model is frozen: the kernel does its own walk over
            # the records and reads the planes and lines the forward read
            rays_o, rays_d = ctx.saved_tensors[14:]
            g, R = _vm_geom(kt)
            go = torch.empty((N, 3), dtype=torch.float32, device=dev)
            gd = torch.empty((N, 3), dtype=torch.float32, device=dev)
            gw = g_w.contiguous() if g_w is not None else torch.zeros(M3, dtype=torch.float32, device=dev)
            with L.device_of(start):
                L.call('dvgo_march_vm_ray_bwd', rec2, n2, stride, off3, N, start, dirs, cfg.stepdist, cfg.xyz_min_h, cfg.xyz_max_h,
                       last, cfg.interval, rays_o, rays_d, cfg.near, cfg.far, *g, R, gw,
                       g_last.contiguous() if g_last is not None else None,
                       g_pts.contiguous() if g_pts is not None else None, go, gd, stream_of(start))
            go, gd = (go if ctx.needs_input_grad[0] else None), (gd if ctx.needs_input_grad[1] else None)
        if not any(needs):
            return (go, gd) + (None,) * 9
        grads = _vm_grad_buffers(kt)                  # one zero fill for the six
        if M2 > 0:
            gw, gl, g_raw, xyz2 = _record_grads(g_w, g_last, M3, M2, dev)
            with L.device_of(start):
                L.call('dvgo_march_vm_density_bwd', rec2, n2, n_steps, stride, off3, off2, N, start, dirs, cfg.stepdist, last,
                       cfg.interval, gw, gl, g_raw, xyz2, stream_of(start))
            vm_density_bwd(g_raw, kt[:3], kt[3:], grads[:3], grads[3:], xyz2, cfg.xyz_min_t, cfg.xyz_max_t)
        return (go, gd, None, None, None, *[b if need else None for b, need in zip(grads, needs)])


def fused_march_vm(density_planes, density_lines, rays_o, rays_d, cfg, raygrad=False):
    """`fused_march(..., positions=True)` over a vector-matrix decomposed density (csrc/march_vm.hip) -> weights [M3],
    raw_alpha [M3], alphainv_last [N], pts [M3,3], ray_id, step_id [M3], off3 [N+1].  `density_planes` / `density_lines`: as
    `ops.vm_density` takes them; gradients flow into the six tensors (the per-record gradient of the raw density, then
    ops.vm_density_bwd).  The result does not depend on their layout.
    Returns None when no fixed record stride exists for `cfg` (`_rec_stride`: an infinite `far`, or scratch over the
    budget): the caller then takes its op-by-op path.  NDC sampling and rays that require grad are refused, the latter unless
    `raygrad=True`: then the forward is the same launches and the same bits, the returned positions are differentiable, and
    the backward launches dvgo_march_vm_ray_bwd first (csrc/march_raygrad.hip: per record the raw-density gradient through
    the position derivative of planes times lines, plus the gradient that arrived for the positions, summed per ray; it
    runs also when none of the six tensors takes a gradient).  The stop-gradients are DirectVoxGO._forward_raygrad's."""
    if cfg.ndc_samples > 0:
        raise NotImplementedError('fused_march_vm: NDC sampling is not built for the decomposed density')
    if not raygrad and torch.is_grad_enabled() and (rays_o.requires_grad or rays_d.requires_grad):
        raise NotImplementedError('fused_march_vm: rays that require grad are not differentiated through the decomposed density')
    stride = _rec_stride(cfg, rays_o.shape[0])
    if stride == 0:
        return None
    return _FusedMarchVM.apply(rays_o.contiguous(), rays_d.contiguous(), cfg, stride, bool(raygrad),
                               *_plane_list(density_planes), *_plane_list(density_lines))


class ContractMarchConfig(_MarchConstants):
    """Host-side constants of one DirectContractedVoxGO render setting, beside `MarchConfig`: the foreground box as centre and
    radius, the distance table `t_tab` [n_max] (device, float32) and the thinning distance `thin_thres` of
    dcvgo.contracted_t_table / thinning_threshold, `bg_len`, the norm ('inf' | 'l2'), the CONTRACTED bounds of the grids,
    the activation's constants and the occupancy mask with its scale / shift."""

    def __init__(self, center, radius, t_tab, bg_len, contracted_norm, thin_thres, xyz_min, xyz_max, act_shift, interval,
                 fast_color_thres, mask=None, xyz2ijk_scale=None, xyz2ijk_shift=None):
        if contracted_norm not in ('inf', 'l2'):
            raise ValueError(f"contracted_norm must be 'inf' or 'l2', got {contracted_norm!r}")
        if t_tab.dim() != 1 or t_tab.dtype != torch.float32 or not t_tab.is_contiguous():
            raise RuntimeError('t_tab must be a contiguous float32 vector')
        super().__init__(xyz_min, xyz_max, act_shift, interval, fast_color_thres, mask, xyz2ijk_scale, xyz2ijk_shift)
        self.center_h, self.radius_h = f3(center), f3(radius)
        self.t_tab, self.n_max = t_tab, int(t_tab.shape[0])
        self.bg_len, self.l2 = float(bg_len), 1 if contracted_norm == 'l2' else 0
        self.thin_thres = float(thin_thres)


class _FusedMarchContract(torch.autograd.Function):
    """csrc/march_contract.hip: the march of DirectContractedVoxGO.  Two host-visible counts, read together: M3 (kept samples,
    sizes the outputs) and M2 (records, sizes the backward's per-record gradient)."""

    @staticmethod
    def forward(ctx, density, rays_o, rays_d, cfg, raygrad=False):
        for x, n in ((rays_o, 'rays_o'), (rays_d, 'rays_d'), (density, 'density'), (cfg.t_tab, 't_tab')):
            check_input(x, n); check_f32(x, n)
        C, X, Y, Z = _grid_geom(density)[:4]
        if C != 1:
            raise RuntimeError('density must be [1,1,X,Y,Z]')
        dev = rays_o.device
        N, stride = rays_o.shape[0], cfg.n_max
        st = stream_of(rays_o)
        n2 = torch.empty(N, dtype=torch.int32, device=dev)
        n3 = torch.empty(N, dtype=torch.int32, device=dev)
        last = torch.empty(N, dtype=torch.float32, device=dev)
        off3 = torch.empty(N + 1, dtype=torch.int64, device=dev)
        off2 = torch.zeros(N + 1, dtype=torch.int64, device=dev)
        rec2 = torch.empty((max(stride * N, 1), 4), dtype=torch.float32, device=dev)
        mask = cfg.mask
        mshape = mask.shape if mask is not None else (0, 0, 0)
        with L.device_of(rays_o):
            L.call('dvgo_march_contract_density', rays_o, rays_d, N, cfg.center_h, cfg.radius_h, cfg.t_tab, cfg.n_max, cfg.bg_len,
                   cfg.l2, cfg.thin_thres, mask, mshape[0], mshape[1], mshape[2], cfg.scale_h, cfg.shift_h, density, X, Y, Z,
                   cfg.xyz_min_h, cfg.xyz_max_h, cfg.act_shift, cfg.interval, cfg.thres, stride, rec2, n2, n3, last, st)
            # (the table's steps are not uniform: rays_o / rays_d stand in for the gather's start / direction)
            M3, M2, ray_id, step_id, weights, alpha = _records_to_samples(rec2, n2, n3, off3, off2, N, stride, cfg, st, rays_o,
                                                                          rays_d, 1.0)
            q = torch.empty((M3, 3), dtype=torch.float32, device=dev)
            t = torch.empty(M3, dtype=torch.float32, device=dev)
            L.call('dvgo_contract_positions', rays_o, rays_d, N, cfg.center_h, cfg.radius_h, cfg.t_tab, cfg.n_max, cfg.bg_len,
                   cfg.l2, ray_id, step_id, M3, q, t, st)
        ctx.cfg, ctx.counts, ctx.geom = cfg, (stride, N, M2, M3), (X, Y, Z)
        ctx.raygrad = bool(raygrad)
        ctx.save_for_backward(rec2, n2, off3, off2, last, rays_o, rays_d, density)
        ctx.mark_non_differentiable(alpha, q, ray_id, step_id, t, off3)
        ctx.set_materialize_grads(False)
        return weights, alpha, last, q, ray_id, step_id, t, off3

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_w, _g_alpha, g_last, _g_q, _g_rid, _g_sid, _g_t, _g_off):
        # the rays' gradient (raygrad=True): wanted also when the model is frozen and `density` takes none
        want_rays = ctx.raygrad and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        want_density = ctx.needs_input_grad[0]
        if not want_density and not want_rays:
            return None, None, None, None, None
        rec2, n2, off3, off2, last, rays_o, rays_d, density = ctx.saved_tensors
        stride, N, M2, M3 = ctx.counts
        cfg, (X, Y, Z) = ctx.cfg, ctx.geom
        dev = rays_o.device
        grad_density = torch.zeros_like(density, memory_format=torch.contiguous_format) if want_density else None
        grad_o = grad_d = None
        if M2 > 0 and (g_w is not None or g_last is not None):
            gw, gl, g_raw, q2 = _record_grads(g_w, g_last, M3, M2, dev)
            with L.device_of(rays_o):
                st = stream_of(rays_o)
                L.call('dvgo_march_contract_density_bwd', rec2, n2, stride, off3, off2, N, rays_o, rays_d, cfg.center_h,
                       cfg.radius_h, cfg.t_tab, cfg.n_max, cfg.bg_len, cfg.l2, last, cfg.interval, gw, gl, g_raw, q2, st)
                if want_density:
                    L.call('dvgo_grid_sample_bwd', g_raw, 1, X, Y, Z, X * Y * Z, Y * Z, Z, 1, q2, cfg.xyz_min_t, cfg.xyz_max_t,
                           M2, grad_density, st)
                if want_rays:
                    # dL/dq2 per record through the density's trilinear sample, then the contraction and the ray (the k0 term
                    # arrives separately: ops.contract_points on the march's q)
                    g_q2 = torch.empty((M2, 3), dtype=torch.float32, device=dev)
                    grad_o = torch.empty((N, 3), dtype=torch.float32, device=dev)
                    grad_d = torch.empty((N, 3), dtype=torch.float32, device=dev)
                    L.call('dvgo_grid_sample_bwd_xyz', density, 1, X, Y, Z, X * Y * Z, Y * Z, Z, 1, g_raw, q2, cfg.xyz_min_t,
                           cfg.xyz_max_t, M2, g_q2, st)
                    L.call('dvgo_contract_ray_bwd_rec', rays_o, rays_d, N, cfg.center_h, cfg.radius_h, cfg.t_tab, cfg.n_max,
                           cfg.bg_len, cfg.l2, rec2, n2, stride, off2, g_q2, M2, grad_o, grad_d, st)
        return (grad_density, grad_o if ctx.needs_input_grad[1] else None, grad_d if ctx.needs_input_grad[2] else None, None,
                None)


def fused_march_contract(density, rays_o, rays_d, cfg, raygrad=False):
    """The fused march of DirectContractedVoxGO (csrc/march_contract.hip) -> weights [M3], raw_alpha [M3], alphainv_last [N],
    q [M3,3] (contracted positions), ray_id, step_id [M3], t [M3], off3 [N+1].  `density` [1,1,X,Y,Z]; `cfg` a
    `ContractMarchConfig`.  One launch marches, `dvgo_march_gather` (no feature grid) and `dvgo_contract_positions` write the
    kept samples; one host read (M3 and M2 together).  The gradient flows into `density`: one raw-density gradient per
    record, then the existing trilinear scatter `dvgo_grid_sample_bwd`.
    Returns None when the fixed-stride records (n_max * N * 16 B) exceed `_MAX_STRIDE_SCRATCH_BYTES`: the caller then takes its
    op-by-op path.
    Rays that require grad are refused unless `raygrad=True`.  Then the forward is the same launches and the backward also
    returns the rays' gradient through `weights` and `alphainv_last`: the per-record raw-density gradients (formed even when
    `density` itself takes no gradient) -> `dvgo_grid_sample_bwd_xyz` (C = 1) at the records' positions -> the contraction's and
    the ray's Jacobian summed per ray, `dvgo_contract_ray_bwd_rec` (csrc/contract_raygrad.hip).  The returned `q` stays
    non-differentiable: a caller that samples further grids at it wraps it in `ops.contract_points`, and autograd adds the two
    pairs of ray gradients.  The table, the kept set and `t` are constants."""
    if not raygrad and torch.is_grad_enabled() and (rays_o.requires_grad or rays_d.requires_grad):
        raise NotImplementedError('fused_march_contract: rays that require grad are not differentiated through the contraction')
    if cfg.n_max * rays_o.shape[0] * 16 > _MAX_STRIDE_SCRATCH_BYTES:
        return None
    return _FusedMarchContract.apply(density.contiguous(), rays_o.contiguous(), rays_d.contiguous(), cfg, bool(raygrad))


class _Composite(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weights, rgb, alphainv_last, ray_id, off3, bg, m_dev=None):
        N = alphainv_last.shape[0]
        rgb = rgb.contiguous()
        weights = weights.contiguous()
        last = alphainv_last.contiguous()
        out = torch.empty((N, 3), dtype=torch.float32, device=weights.device)
        with L.device_of(weights):
            L.call('dvgo_march_composite', weights, rgb, None, off3, N, last, float(bg), out, None, stream_of(weights))
        ctx.save_for_backward(weights, rgb, ray_id)
        ctx.bg = float(bg)
        ctx.N = N
        ctx.m_dev = m_dev
        # A loss that also consumes `rgb` / `alphainv_last` (run.py:381-385: rgbper, entropy) may leave its gradient of
        # them in `ctx.extra` instead of returning it to autograd (train._FusedLoss does, after checking these two
        # addresses): the backward below then adds to it in place -- one gradient per tensor, no summation launches.
        ctx.rgb_ptr, ctx.last_ptr = rgb.data_ptr(), last.data_ptr()
        ctx.extra = None
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        weights, rgb, ray_id = ctx.saved_tensors
        g = g.contiguous()
        want_rgb, want_last = ctx.needs_input_grad[1], ctx.needs_input_grad[2]

        def bwd(gw, grgb, glast, accumulate):
            with L.device_of(weights):
                L.call('dvgo_march_composite_bwd', g, weights, rgb, ray_id, weights.shape[0], ctx.m_dev, ctx.N, ctx.bg, gw,
                       grgb, glast, accumulate, stream_of(weights))

        gw = torch.empty_like(weights) if ctx.needs_input_grad[0] else None
        # the loss's gradients of rgb / alphainv_last (either may be None), to be added to; else fresh ones
        (grgb, glast), accumulate = (ctx.extra, 1) if ctx.extra is not None else ((None, None), 0)
        ctx.extra = None
        g2 = torch.empty_like(rgb) if grgb is None and want_rgb else None
        l2 = torch.empty(ctx.N, dtype=torch.float32, device=g.device) if glast is None and want_last else None
        if not accumulate:
            bwd(gw, g2, l2, 0)
        else:
            if g2 is not None or l2 is not None:    # only one of the two was handed over: finish the other the plain way
                bwd(None, g2, l2, 0)
            bwd(gw, grgb, glast, 1)
        return gw, (grgb if grgb is not None else g2), (glast if glast is not None else l2), None, None, None, None


def composite(weights, rgb, alphainv_last, ray_id, off3, bg, m_dev=None):
    """rgb_marched = segment_sum(weights * rgb) + alphainv_last * bg   (lib/dvgo.py:554-559)"""
    return _Composite.apply(weights, rgb, alphainv_last, ray_id, off3, bg, m_dev)


@torch.no_grad()
def composite_depth(weights, step_id, off3, n_rays):
    """depth = segment_sum(weights * step_id)   (lib/dvgo.py:569-576, no_grad in the reference)"""
    dev = weights.device
    dummy_rgb = torch.zeros((weights.shape[0], 3), dtype=torch.float32, device=dev)
    zeros = torch.zeros(n_rays, dtype=torch.float32, device=dev)
    out = torch.empty((n_rays, 3), dtype=torch.float32, device=dev)
    depth = torch.empty(n_rays, dtype=torch.float32, device=dev)
    with L.device_of(weights):
        L.call('dvgo_march_composite', weights.contiguous(), dummy_rgb, step_id, off3, n_rays, zeros, 0.0, out, depth,
               stream_of(weights))
    return depth
