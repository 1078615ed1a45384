"""Data-parallel reduction of the grid gradients of one training step (train.TrainStep, world > 1):
every collective a step issues outside `fused.brick_union`.  TrainStep calls start() after the backward, wait() before the
TV add-grad and finish() before optimizer.step(), then waits for the handles of finish()."""
import torch
import torch.distributed as dist
import torch.nn as nn


def flat_view(t):
    """1-D view of a dense tensor's memory (no copy): collectives want plain contiguous buffers, and the
    feature grid / its gradient are stored channels-last."""
    if t.is_contiguous():
        return t.view(-1)
    if t.dim() == 5 and t.is_contiguous(memory_format=torch.channels_last_3d):
        v = t.permute(0, 2, 3, 4, 1).reshape(-1)
        assert v.data_ptr() == t.data_ptr()
        return v
    return None


class GridReducer:
    # A batch of rays touches the voxels along those rays only: on a trained scene a few per cent of the grid, while
    # the dense all-reduce always moves all of it (213 MB at 160^3 -- more than a whole step of compute on such
    # scenes).  The touched set differs per rank, so: OR-reduce a byte mask (4 MB), compact the union's rows
    # [n, C + 1] (features + density), all-reduce that, write back.  Untouched voxels stay exactly zero on every
    # rank, which is what the masked Adam and the sparse TV branch on.  Used while the union stays below
    # TOUCHED_MAX of the grid (decided from the previous union, identical on all ranks; re-probed every
    # PROBE_EVERY steps while the dense path is in use).
    TOUCHED_MAX = 0.35
    BRICK_SPARSE_MAX = 0.5
    PROBE_EVERY = 64

    def __init__(self, model, optimizer, process_group, shard_grids, small):
        self.model, self.optimizer, self.pg, self._small = model, optimizer, process_group, small
        self.world, self.rank = dist.get_world_size(process_group), dist.get_rank(process_group)
        # dense scenes: reduce-scatter the grid gradients, update only the owned slab, all-gather the parameters (see
        # _grid_shards); False = plain all-reduce + full update on every rank
        self.shard_grids = shard_grids
        self._touched_frac = None            # fraction of voxels in the last union; None: not probed yet
        self._steps_since_probe = 0
        self.last_mode = None                 # 'bricks' / 'sharded' / 'allreduce' / 'touched': what the last step used
        self.last_wire_bytes = 0
        # the sharded update leaves every rank with the moments of its own X-slab only: before any step that updates the
        # whole grid on every rank (tiles, touched voxels, all-reduce fallback) the slabs are gathered once
        self._moments_sharded = False
        self._works, self._shards = [], None
        optimizer._dvgo_reducer = self        # (checkpoint.save_checkpoint gathers the slabs before it writes)

    def start(self, tile_bytes, probe):
        """After the backward.  `tile_bytes` not None: the brick kernel has applied the all-reduced tiles (that many bytes
        travelled inside fused.brick_union; nothing left to reduce); `probe`: the compacted touched-voxel reduction may
        be tried."""
        self.last_mode, self.last_wire_bytes, self._works, self._shards = None, 0, [], None
        if tile_bytes is not None:
            self.last_mode, self.last_wire_bytes = 'bricks', tile_bytes
            return
        # every rank must enter the same collectives: a rank whose shard produced no gradient for a grid brings zeros
        for p in (getattr(self.model, 'density', None), getattr(self.model, 'k0', None)):
            if isinstance(p, nn.Parameter) and p.requires_grad and p.grad is None:
                p.grad = torch.zeros_like(p, memory_format=torch.preserve_format)
        pending = self._touched_start() if probe else None
        if pending is not None:
            self._works = [pending]
            self.whole_grid_update_ahead()
            self.last_mode = 'touched'
            return
        self._shards = self._grid_shards()
        if self._shards:
            self._works = [dist.reduce_scatter_tensor(fg[lo:hi], fg, op=dist.ReduceOp.SUM, group=self.pg, async_op=True)
                           for _, _, fg, lo, hi, _ in self._shards]
            self.last_mode = 'sharded'
        else:
            self.whole_grid_update_ahead()
            self._works = self._all_reduce_grids()
            self.last_mode = 'allreduce'

    def wait(self):
        """The small bucket, then the grid gradients are reduced.  Returns the keyword of the TV add-grad: a rank that owns
        a slab adds the TV gradient of that slab."""
        self._reduce_small()
        for wk in self._works:
            wk.wait()
        return {'x_range': self._shards[0][5]} if self._shards else {}

    def finish(self):
        """Sharded: Adam on the owned slabs, then the parameters travel.  Returns the all-gather handles."""
        works = []
        for p, fp, fg, lo, hi, _ in self._shards or ():
            self._moments_sharded = True
            self.optimizer.step_shard(p, fp, fg, lo, hi)
            p.grad = None                      # consumed: optimizer.step() below skips the grids
            works.append(dist.all_gather_into_tensor(fp, fp[lo:hi], group=self.pg, async_op=True))
        return works

    def _touched_start(self):
        """Sparse scenes: start the compacted touched-voxel reduction (see _reduce_touched); returns its handle, or None
        when the dense path (sharded reduce-scatter / all-reduce) has to take the step."""
        self._steps_since_probe += 1
        probe = self._touched_frac is None or self._steps_since_probe >= self.PROBE_EVERY
        rd = self._rows() if (probe or self._touched_frac <= self.TOUCHED_MAX) else None
        return self._reduce_touched(*rd) if rd is not None else None

    def _all_reduce_grids(self):
        """Plain sum of the full grid gradients on every rank (the fallback when the grids cannot be sharded)."""
        works = []
        for p in (self.model.density, self.model.k0):
            if p.grad is not None:
                flat = flat_view(p.grad)
                if flat is not None:
                    works.append(dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=self.pg, async_op=True))
                else:                                 # exotic strides: staged through a contiguous copy
                    tmp = p.grad.contiguous()
                    dist.all_reduce(tmp, op=dist.ReduceOp.SUM, group=self.pg)
                    p.grad.copy_(tmp)
        return works

    def _rows(self):
        """(k0.grad as [n_vox, C] rows, density.grad as [n_vox]) when both share the lattice and are row-addressable."""
        d, k = self.model.density.grad, self.model.k0.grad
        if d is None or k is None or d.dim() != 5 or k.dim() != 5 or d.shape[2:] != k.shape[2:] or not d.is_contiguous():
            return None
        flat = flat_view(k) if k.is_contiguous(memory_format=torch.channels_last_3d) else None
        if flat is None:
            return None
        return flat.view(-1, k.shape[1]), d.view(-1)

    def _reduce_touched(self, rows, dflat):
        mask = (rows != 0).any(1) | (dflat != 0)
        m8 = mask.to(torch.uint8)
        dist.all_reduce(m8, op=dist.ReduceOp.MAX, group=self.pg)
        idx = m8.nonzero().flatten()                       # the union, identical on every rank (one host read)
        self._touched_frac = idx.numel() / max(m8.numel(), 1)
        self._steps_since_probe = 0
        if self._touched_frac > self.TOUCHED_MAX:
            return None                                     # dense scene: the caller falls back to the plain all-reduce
        C = rows.shape[1]
        compact = torch.empty((idx.numel(), C + 1), dtype=rows.dtype, device=rows.device)
        if idx.numel():
            compact[:, :C] = rows[idx]
            compact[:, C] = dflat[idx]
        work = dist.all_reduce(compact, op=dist.ReduceOp.SUM, group=self.pg, async_op=True)

        class _Pending:
            def wait(_self):
                work.wait()
                if idx.numel():
                    rows[idx] = compact[:, :C]
                    dflat[idx] = compact[:, C]
        return _Pending()

    # ------------------------------------------------------------------------------------------------------------
    # Dense scenes (every voxel has a gradient: the roofline case): a plain all-reduce moves 2 (P-1)/P x 213 MB per rank
    # AND leaves every rank sweeping all 53 M elements through Adam.  Instead (ZeRO-1 style):
    #   reduce_scatter   rank r receives the SUM of the gradient of the X-planes [r X/P, (r+1) X/P) -- in place, the slab
    #                    is a contiguous range of the gradient's memory (channels-last / C == 1: X is the outermost axis)
    #   TV + Adam        on that slab only (1/P of the optimizer's traffic; the TV stencil reads the replicated params)
    #   all_gather       the updated parameter slabs, in place in the parameters
    # Same bytes on the wire as the all-reduce ((P-1)/P x 213 MB out and in per rank and phase, spread over all xGMI
    # links by RCCL), 1/P of the optimizer work, and the parameters -- not the gradients -- are what ends up replicated.
    # ------------------------------------------------------------------------------------------------------------
    def _sharded_grids(self):
        """(density, k0) when the sharded update is on and the optimizer can run it; else ()."""
        if not (self.shard_grids and hasattr(self.optimizer, 'step_shard')):
            return ()
        return getattr(self.model, 'density', None), getattr(self.model, 'k0', None)

    def _grid_shards(self):
        """[(param, flat param, flat grad, lo, hi, (x_lo, x_hi))] for the grids when the sharded update applies."""
        rank, out = self.rank, []
        for p in self._sharded_grids():
            if not isinstance(p, nn.Parameter) or p.grad is None or p.dim() != 5:
                return None
            x_outermost = p.shape[1] == 1 and p.is_contiguous() or p.is_contiguous(memory_format=torch.channels_last_3d)
            fp, fg = flat_view(p.data), flat_view(p.grad)
            X = p.shape[2]
            if not x_outermost or fp is None or fg is None or p.grad.stride() != p.stride() or X % self.world != 0:
                return None
            n = fp.numel() // self.world
            out.append((p, fp, fg, rank * n, (rank + 1) * n, (rank * (X // self.world), (rank + 1) * (X // self.world))))
        return out

    @torch.no_grad()
    def gather_optimizer_state(self):
        """Data-parallel runs with the sharded update: every rank has only ever updated the moments of the X-slab it
        owns.  Before `checkpoint.save_checkpoint` (or any other reader of `optimizer.state_dict()`), all-gather the slabs
        in place so that every rank holds the complete `exp_avg` / `exp_avg_sq` of both grids -- the state a single
        process would have written (run.py:420-437).  No-op when the grids are not sharded."""
        grids, rank, done = self._sharded_grids(), self.rank, False
        if not grids:
            return False
        for p in grids:
            st = self.optimizer.state.get(p) if isinstance(p, nn.Parameter) else None
            if not st or p.dim() != 5 or p.shape[2] % self.world != 0:
                continue
            for key in ('exp_avg', 'exp_avg_sq'):
                flat = flat_view(st[key])
                if flat is None or st[key].stride() != p.stride():
                    raise RuntimeError(f'gather_optimizer_state: {key} is not laid out like its parameter')
                n = flat.numel() // self.world
                dist.all_gather_into_tensor(flat, flat[rank * n:(rank + 1) * n].clone(), group=self.pg)
            done = True
        self._moments_sharded = False
        return done

    def whole_grid_update_ahead(self):
        """Call (on every rank: it is a collective when it does anything) before a step in which every rank updates the
        WHOLE grid: after sharded steps each rank only holds current moments for its own slab.  Also what
        `checkpoint.save_checkpoint` calls before it writes."""
        if self._moments_sharded:
            self.gather_optimizer_state()

    def _reduce_small(self):
        """One flat bucket for the handful of MLP gradients."""
        small = [p for p in self._small if p.grad is not None]
        if small:
            flat = torch.cat([p.grad.reshape(-1) for p in small])
            dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=self.pg)
            off = 0
            for p in small:
                n = p.grad.numel()
                p.grad.copy_(flat[off:off + n].view_as(p.grad))
                off += n
