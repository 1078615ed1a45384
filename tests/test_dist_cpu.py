"""CPU, world_size 2, gloo: the ray-parallel data-parallel step.

The HIP ops need a GPU, so the N > 1 *host logic* is exercised with a small pure-torch stand-in model
that returns the same result dict as DirectVoxGO.forward: rays sharded by rank, every loss term
normalised by the global ray count, grid gradients summed with all-reduce, MLP gradients in one flat
bucket, optimizer step after the reduction.  Two ranks on half the batch each must end at exactly the
parameters one process reaches on the whole batch.
"""
import contextlib
import os
import socket

import pytest
import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn
import torch.nn.functional as F

from directvoxgo_amd.train import FINE_TRAIN, TrainStep, render_loss


class ToyModel(nn.Module):
    """Same parameter names / result dict as DirectVoxGO, pure torch, S fixed samples per ray."""

    def __init__(self, S=6):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        self.density = nn.Parameter(torch.randn(1, 1, 6, 5, 5, generator=g))
        self.k0 = nn.Parameter((torch.randn(1, 6, 6, 5, 5, generator=g) * 0.3).contiguous(memory_format=torch.channels_last_3d))
        self.rgbnet = nn.Sequential(nn.Linear(6, 8), nn.ReLU(), nn.Linear(8, 3))
        for p in self.rgbnet.parameters():
            p.data = torch.randn(p.shape, generator=g) * 0.3
        self.S = S

    def forward(self, rays_o, rays_d, viewdirs, global_step=None, bg=1, **kw):
        N = rays_o.shape[0]
        t = torch.linspace(0.1, 0.9, self.S)
        pts = rays_o[:, None] + rays_d[:, None] * t[None, :, None]                  # [N,S,3] in [-1,1]
        grid = pts.reshape(1, 1, 1, -1, 3).flip(-1)
        dens = F.grid_sample(self.density, grid, align_corners=True).reshape(-1)
        feat = F.grid_sample(self.k0, grid, align_corners=True).reshape(6, -1).T
        alpha = (1 - torch.exp(-F.softplus(dens))).reshape(N, self.S)
        T = torch.cumprod(torch.cat([torch.ones(N, 1), 1 - alpha + 1e-10], 1), 1)
        weights = (T[:, :-1] * alpha).reshape(-1)
        rgb = torch.sigmoid(self.rgbnet(feat))
        ray_id = torch.arange(N).repeat_interleave(self.S)
        marched = torch.zeros(N, 3).index_add(0, ray_id, weights[:, None] * rgb) + T[:, -1:] * bg
        return {'alphainv_last': T[:, -1], 'weights': weights, 'rgb_marched': marched, 'raw_alpha': alpha.reshape(-1),
                'raw_rgb': rgb, 'ray_id': ray_id}


def make_batch(n):
    g = torch.Generator().manual_seed(11)
    ro = torch.rand(n, 3, generator=g) * 0.4 - 0.2
    rd = torch.rand(n, 3, generator=g) * 1.2 - 0.6
    return ro, rd, rd / rd.norm(dim=-1, keepdim=True), torch.rand(n, 3, generator=g)


class TorchMaskedAdam(torch.optim.Optimizer):
    """MaskedAdam's interface (param-group key `skip_zero_grad`, `step`, `step_shard`) on torch CPU ops
    (oracle/torch_cpu.adam_step = lib/masked_adam.py:39-71 over adam_upd_kernel.cu:8-58): the stand-in that lets the
    sharded data-parallel update of TrainStep run without a GPU."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.99), eps=1e-8):
        super().__init__(params, {'lr': lr, 'betas': betas, 'eps': eps})

    def _st(self, p):
        st = self.state[p]
        if not st:
            st.update(step=0, exp_avg=torch.zeros_like(p, memory_format=torch.preserve_format),
                      exp_avg_sq=torch.zeros_like(p, memory_format=torch.preserve_format))
        return st

    def _group_of(self, p):
        return next(g for g in self.param_groups if any(q is p for q in g['params']))

    @torch.no_grad()
    def step(self):
        from oracle.torch_cpu import adam_step
        for g in self.param_groups:
            for p in g['params']:
                if p.grad is None:
                    continue
                st = self._st(p)
                st['step'] += 1
                adam_step(p.data, p.grad, st['exp_avg'], st['exp_avg_sq'], st['step'], g['lr'], mode=1 if g.get('skip_zero_grad') else 0)

    @torch.no_grad()
    def step_shard(self, p, flat_p, flat_g, lo, hi):
        from directvoxgo_amd.train import flat_view
        from oracle.torch_cpu import adam_step
        g, st = self._group_of(p), self._st(p)
        st['step'] += 1
        adam_step(flat_p[lo:hi], flat_g[lo:hi], flat_view(st['exp_avg'])[lo:hi], flat_view(st['exp_avg_sq'])[lo:hi], st['step'],
                  g['lr'], mode=1 if g.get('skip_zero_grad') else 0)


@contextlib.contextmanager
def record_collectives(log):
    """Append (name, reduce op, dtype, numel of the whole buffer) to `log` for every collective issued inside."""
    whole = {'all_reduce': 0, 'reduce_scatter_tensor': 1, 'all_gather_into_tensor': 0}     # (output, input) argument order
    saved = {name: getattr(dist, name) for name in whole}

    def wrap(name):
        def call(*args, **kw):
            op = kw.get('op', None if name == 'all_gather_into_tensor' else dist.ReduceOp.SUM)
            t = args[whole[name]]
            log.append((name, None if op is None else str(op).split('.')[-1], str(t.dtype).split('.')[-1], t.numel()))
            return saved[name](*args, **kw)
        return call
    for name in whole:
        setattr(dist, name, wrap(name))
    try:
        yield
    finally:
        for name, fn in saved.items():
            setattr(dist, name, fn)


def run_steps(model, batch, rank, world, n_steps=3, mode='dense', out=None, schedule=None):
    cfg = dict(FINE_TRAIN, weight_entropy_last=0.01, weight_rgbper=0.05)
    if mode in ('sharded', 'sharded_off', 'flip'):
        # Adam with the masked rule on the grids, the sharded update on (reduce-scatter -> slab Adam -> all-gather)
        # or off (all-reduce -> full Adam on every rank)
        opt = TorchMaskedAdam([{'params': [model.density], 'lr': 0.1, 'skip_zero_grad': True},
                               {'params': [model.k0], 'lr': 0.1, 'skip_zero_grad': True},
                               {'params': list(model.rgbnet.parameters()), 'lr': 1e-2}])
        step = TrainStep(model, cfg, dict(bg=1), optimizer=opt, touched_reduce=False, shard_grids=(mode != 'sharded_off'))
    else:
        opt = torch.optim.SGD(model.parameters(), lr=0.5)
        step = TrainStep(model, cfg, dict(bg=1), optimizer=opt, touched_reduce=(mode != 'dense'))
    reducer = step.dp                     # dp.GridReducer: the thresholds live there; None in the one-process reference
    if mode == 'touched':
        reducer.TOUCHED_MAX = 2.0         # always take the compact (touched-voxel) reduction
    elif mode == 'adaptive':
        reducer.TOUCHED_MAX = 0.0         # probe, find the union too large, fall back to the dense all-reduce
    n = batch[0].shape[0] // world
    shard = tuple(t[rank * n:(rank + 1) * n] for t in batch)
    losses = []
    modes_seen = []
    for s in range(n_steps):
        if mode == 'flip' and s == 2:
            # the reduction mode changes mid-run -- two sharded steps (each rank updates the moments of its
            # own X-slab only), then the compacted touched-voxel reduction with a full update on every rank
            step.touched_reduce = True
            if reducer is not None:
                reducer.TOUCHED_MAX = 2.0
        with record_collectives([] if schedule is None else schedule.setdefault(f'step {s}', [])):
            losses.append(step(*shard, global_step=s))
        modes_seen.append(step.last_mode)
    if mode == 'flip' and world > 1:
        assert modes_seen == ['sharded', 'sharded', 'touched', 'touched'], modes_seen
    if mode == 'sharded' and world > 1:
        assert modes_seen == ['sharded'] * n_steps, modes_seen  # the slab path really ran
    if mode == 'sharded_off':
        assert 'sharded' not in modes_seen, modes_seen
    if out is not None:
        out['step'] = step
    return torch.stack(losses)


def _moments(model, step):
    return {f'{name}.{key}': step.optimizer.state[p][key].detach().numpy().copy()
            for name, p in (('density', model.density), ('k0', model.k0)) for key in ('exp_avg', 'exp_avg_sq')}


def _worker(rank, world, port, q, mode='dense'):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(1)
    model = ToyModel()
    out = {}
    losses = run_steps(model, make_batch(32), rank, world, mode=mode, out=out, n_steps=4 if mode == 'flip' else 3)
    dist.all_reduce(losses)           # per-rank shares of the global loss add up to it
    moments = None
    if mode == 'flip':                # after the flip every rank holds the complete, identical state
        for p in (model.density, model.k0):
            for key in ('exp_avg', 'exp_avg_sq'):
                mine = out['step'].optimizer.state[p][key].clone()
                other = mine.clone()
                dist.all_reduce(other, op=dist.ReduceOp.MAX)
                assert torch.equal(mine, other), f'ranks disagree on {key}'
        moments = _moments(model, out['step'])
    if mode == 'sharded':             # what a checkpoint of a data-parallel run needs: every rank's slab of the moments:
        from directvoxgo_amd.checkpoint import save_checkpoint        # the save helper gathers them itself
        assert out['step'].dp._moments_sharded
        save_checkpoint(None, model, out['step'].optimizer, 3)        # (path None: this rank does not write)
        assert not out['step'].dp._moments_sharded
        moments = _moments(model, out['step'])
    if rank == 0:
        # numpy: pickled by value (torch tensors would travel as shared-memory handles of a process about to exit)
        q.put(({k: v.detach().numpy().copy() for k, v in model.state_dict().items()}, losses.numpy().copy(), moments))
    dist.barrier()
    dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.timeout(120)
@pytest.mark.parametrize('mode', ['dense', 'touched', 'adaptive', 'sharded', 'sharded_off', 'flip'])
def test_two_ranks_equal_one_process(mode):
    """`touched`: the grid gradients travel as the compacted union of the voxels either rank touched.
    `sharded`: reduce-scatter of the grid gradients, Adam on the owned X-slab only, all-gather of the parameters."""
    ref_model = ToyModel()
    ref_out = {}
    ref_losses = run_steps(ref_model, make_batch(32), 0, 1, mode=mode if (mode.startswith('sharded') or mode == 'flip') else 'dense',
                           out=ref_out, n_steps=4 if mode == 'flip' else 3)
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, mode)) for r in range(2)]
    for p in procs:
        p.start()
    sd, losses, moments = q.get(timeout=100)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert torch.allclose(torch.from_numpy(losses), ref_losses, rtol=1e-5, atol=1e-7)
    for k, v in ref_model.state_dict().items():
        assert torch.allclose(torch.from_numpy(sd[k]), v, rtol=1e-5, atol=1e-6), k
    if mode in ('sharded', 'flip'):   # gathered moments == the single process's: the checkpoint of the run is complete
        for k, v in _moments(ref_model, ref_out['step']).items():
            assert np.allclose(moments[k], v, rtol=1e-5, atol=1e-8), k
            assert np.abs(moments[k]).sum() > 0


def test_flat_view_of_channels_last_grid_is_a_view():
    from directvoxgo_amd.train import flat_view
    g = torch.randn(1, 12, 5, 6, 7).contiguous(memory_format=torch.channels_last_3d)
    v = flat_view(g)
    assert v is not None and v.is_contiguous() and v.data_ptr() == g.data_ptr() and v.numel() == g.numel()
    v.mul_(2)                                           # writes through to the grid
    assert torch.equal(g.permute(0, 2, 3, 4, 1).reshape(-1), v)
    assert flat_view(torch.randn(1, 1, 4, 4, 4)).numel() == 64
    assert flat_view(torch.randn(4, 6)[:, ::2]) is None


def test_render_loss_equals_reference_formula_on_one_rank():
    """run.py:377-386 written with means == the sum / global-count form used for DP."""
    m = ToyModel()
    ro, rd, vd, tgt = make_batch(16)
    res = m(ro, rd, vd)
    cfg = dict(FINE_TRAIN)
    a = render_loss(res, tgt, 16, cfg)
    b = cfg['weight_main'] * F.mse_loss(res['rgb_marched'], tgt)
    pout = res['alphainv_last'].clamp(1e-6, 1 - 1e-6)
    b = b + cfg['weight_entropy_last'] * (-(pout * torch.log(pout) + (1 - pout) * torch.log(1 - pout)).mean())
    rgbper = (res['raw_rgb'] - tgt[res['ray_id']]).pow(2).sum(-1)
    b = b + cfg['weight_rgbper'] * ((rgbper * res['weights'].detach()).sum() / 16)
    assert torch.allclose(a, b, rtol=1e-6)


def _schedule_worker(rank, world, port, q, mode):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(1)
    model = ToyModel()
    out, schedule = {}, {}
    run_steps(model, make_batch(32), rank, world, mode=mode, out=out, n_steps=4 if mode == 'flip' else 3, schedule=schedule)
    if mode == 'sharded':
        from directvoxgo_amd.checkpoint import save_checkpoint
        with record_collectives(schedule.setdefault('save', [])):
            save_checkpoint(None, model, out['step'].optimizer, 3)
    q.put((rank, schedule))
    dist.barrier()
    dist.destroy_process_group()


# (collective, reduce op, dtype, elements of the whole buffer) as `record_collectives` logs them, for the toy model: density
# 150 voxels, k0 900 elements, the colour MLP 83 parameters, and a union of 64 touched voxels x (6 channels + density)
_ALL_REDUCE = [('all_reduce', 'SUM', 'float32', 150), ('all_reduce', 'SUM', 'float32', 900), ('all_reduce', 'SUM', 'float32', 83)]
_TOUCHED = [('all_reduce', 'MAX', 'uint8', 150), ('all_reduce', 'SUM', 'float32', 448), ('all_reduce', 'SUM', 'float32', 83)]
_SHARDED = [('reduce_scatter_tensor', 'SUM', 'float32', 150), ('reduce_scatter_tensor', 'SUM', 'float32', 900),
            ('all_reduce', 'SUM', 'float32', 83),
            ('all_gather_into_tensor', None, 'float32', 150), ('all_gather_into_tensor', None, 'float32', 900)]
_GATHER_MOMENTS = [('all_gather_into_tensor', None, 'float32', 150), ('all_gather_into_tensor', None, 'float32', 150),
                   ('all_gather_into_tensor', None, 'float32', 900), ('all_gather_into_tensor', None, 'float32', 900)]
SCHEDULE = {
    'dense': {'step 0': _ALL_REDUCE, 'step 1': _ALL_REDUCE, 'step 2': _ALL_REDUCE},
    'touched': {'step 0': _TOUCHED, 'step 1': _TOUCHED, 'step 2': _TOUCHED},
    # the probe of step 0 finds the union too large; no probe again before PROBE_EVERY steps
    'adaptive': {'step 0': [('all_reduce', 'MAX', 'uint8', 150)] + _ALL_REDUCE, 'step 1': _ALL_REDUCE, 'step 2': _ALL_REDUCE},
    'sharded': {'step 0': _SHARDED, 'step 1': _SHARDED, 'step 2': _SHARDED, 'save': _GATHER_MOMENTS},
    'sharded_off': {'step 0': _ALL_REDUCE, 'step 1': _ALL_REDUCE, 'step 2': _ALL_REDUCE},
    # step 2: the slab moments are gathered once the compacted reduction is under way, before the whole-grid update
    'flip': {'step 0': _SHARDED, 'step 1': _SHARDED, 'step 2': _TOUCHED[:2] + _GATHER_MOMENTS + _TOUCHED[2:], 'step 3': _TOUCHED},
}


@pytest.mark.timeout(120)
@pytest.mark.parametrize('mode', ['dense', 'touched', 'adaptive', 'sharded', 'sharded_off', 'flip'])
def test_collective_schedule(mode):
    """Which collectives a step issues, in which order, on what: both ranks log the same list, and it is the list the step
    issued before the reduction moved into dp.GridReducer (recorded with this test on that code).  `save`: the gather of
    the slab moments inside save_checkpoint."""
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_schedule_worker, args=(r, 2, port, q, mode)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=100) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert got[0] == got[1]
    assert got[0] == SCHEDULE[mode]
