"""Cost of one camera-pose iteration on an unbounded scene: DirectContractedVoxGO(raygrad=True) on its two render paths, with
the ray gradient through the contraction from csrc/contract_raygrad.hip, against the same iteration with the contraction
restated in torch ops under autograd -- what a user would write without the kernel.

Scene: scenes.unbounded_scene at --world^3 (its own ground-truth model, frozen; 24 views of --side x --side), every pose turned
by 1 degree and moved by 0.03.  One iteration is what pose.refine_poses runs per step without `train_model`: --rays random
pixels -> CameraRefiner.rays -> model(...) -> train.render_loss -> backward into `delta` -> Adam on `delta`.
  op_by_op     fused_march=False: sampler, ops.contract_points, two position-differentiable trilinear samples
  fused        fused_march=True: the march's backward hands its per-record gradients to dvgo_contract_ray_bwd_rec, the colour
               grid's term goes through ops.contract_points
  torch_ops    op_by_op with ops.contract_points replaced by the contraction written in torch ops on the kept samples
               (gathers of the rays, the norm, torch.where), differentiated by autograd
One process, everything warmed up, the variants alternating within a round, device events around each iteration, the median
over rounds x reps and the spread (max - min of the per-round medians).  The first iteration's delta gradients of the three
variants are compared as well.  Prints one JSON line per measurement; `--out FILE` also writes them there.

  python tools/contract_raygrad_bench.py [--world 64] [--side 32] [--rays 8192] [--reps 10] [--rounds 3] [--out FILE]
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=10, help='timed iterations per variant and round')
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--rays', type=int, default=8192)
ap.add_argument('--world', type=int, default=64)
ap.add_argument('--side', type=int, default=32)
ap.add_argument('--out', default=None)
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from directvoxgo_amd import dcvgo, scenes  # noqa: E402
from directvoxgo_amd.pose import CameraRefiner, se3_exp  # noqa: E402
from directvoxgo_amd.train import COARSE_TRAIN, render_loss  # noqa: E402

assert torch.cuda.is_available(), 'contract_raygrad_bench needs the GPU: a CPU run measures nothing'
VARIANTS = ('op_by_op', 'fused', 'torch_ops')
S = args.side
sc = scenes.unbounded_scene(world=args.world, H=S, W=S, focal=0.75 * S)
model, RK = sc['gt'], sc['render_kwargs']
model.raygrad = True
for p in model.parameters():
    p.requires_grad_(False)
true = torch.from_numpy(sc['train_poses'])[:, :3, :4].float()
n = true.shape[0]
gen = torch.Generator().manual_seed(7)
axis = torch.randn(n, 3, generator=gen)
axis = axis / axis.norm(dim=-1, keepdim=True)
shift = torch.randn(n, 3, generator=gen)
shift = shift / shift.norm(dim=-1, keepdim=True) * 0.03
E = se3_exp(torch.cat([axis * math.radians(1.0), torch.zeros(n, 3)], -1))[:, :, :3]
noisy = torch.cat([E @ true[:, :, :3], true[:, :, 3:] + shift[:, :, None]], -1)
K = np.array([[0.75 * S, 0, 0.5 * S], [0, 0.75 * S, 0.5 * S], [0, 0, 1]], np.float32)
refiner = CameraRefiner(noisy, np.array([[S, S]] * n), np.stack([K] * n)).cuda()
opt = torch.optim.Adam([refiner.delta], lr=1e-5)                 # (the poses stay what they are over the run)
flat = sc['target']
view = torch.randint(n, (args.rays,), generator=gen).cuda()
pix_i = torch.randint(S, (args.rays,), generator=gen).cuda()
pix_j = torch.randint(S, (args.rays,), generator=gen).cuda()
target = flat[view * S * S + pix_j * S + pix_i]
CFG = dict(COARSE_TRAIN, weight_entropy_last=0.0, weight_rgbper=0.0)
kernel_points = dcvgo.contract_points


def torch_points(rays_o, rays_d, ray_id, step_id, q, center, radius, t_tab, bg_len, contracted_norm):
    """ops.contract_points without the kernel: the contraction in torch ops (its values replace the sampler's q)."""
    c, r = model.scene_center, model.scene_radius
    o = (rays_o - c) / r
    u = rays_d / r
    d = u / u.norm(dim=-1, keepdim=True)
    p = o[ray_id] + d[ray_id] * t_tab[step_id].unsqueeze(-1)
    nrm = p.abs().amax(-1) if contracted_norm == 'inf' else p.norm(dim=-1)
    f = (1 + bg_len) / nrm - bg_len / nrm ** 2
    return torch.where((nrm <= 1).unsqueeze(-1), p, p * f.unsqueeze(-1))


def on(variant):
    model.fused_march = variant == 'fused'
    dcvgo.contract_points = torch_points if variant == 'torch_ops' else kernel_points


def iteration(variant, step=True):
    on(variant)
    rays_o, rays_d, viewdirs = refiner.rays(view, pix_i, pix_j)
    res = model(rays_o, rays_d, viewdirs, global_step=None, **RK)
    loss = render_loss(res, target, args.rays, CFG)
    opt.zero_grad(set_to_none=True)
    loss.backward(inputs=[refiner.delta])
    if step:
        opt.step()
    return res


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def summary(rounds):
    meds = [float(np.median(r)) for r in rounds]
    return {'median_ms': round(float(np.median(np.concatenate(rounds))), 4), 'spread_ms': round(max(meds) - min(meds), 4)}


out = [{'reps': args.reps, 'rounds': args.rounds, 'world': args.world, 'views': n, 'side': S, 'rays': args.rays,
        'stepsize': RK['stepsize'], 'bg_len': model.bg_len, 'norm': model.contracted_norm}]
print(json.dumps(out[0]), flush=True)

grads, kept = {}, {}
for v in VARIANTS:
    kept[v] = int(iteration(v, step=False)['ray_id'].shape[0])
    grads[v] = refiner.delta.grad.detach().clone()
scale = float(grads['op_by_op'].abs().max())
out.append({'kept_samples': kept, 'delta_grad_max': scale,
            'delta_grad_difference_over_max': {v: float((grads[v] - grads['op_by_op']).abs().max()) / scale for v in VARIANTS[1:]}})
print(json.dumps(out[-1]), flush=True)

for v in VARIANTS:
    for _ in range(3):
        iteration(v)
torch.cuda.synchronize()
T = {v: [] for v in VARIANTS}
for _ in range(args.rounds):
    for v in VARIANTS:
        ev = [timed(lambda: iteration(v)) for _ in range(args.reps)]
        torch.cuda.synchronize()
        T[v].append([a.elapsed_time(b) for a, b in ev])
row = {'pose_iteration': {v: summary(T[v]) for v in VARIANTS}}
out.append(row)
print(json.dumps(row), flush=True)
on('op_by_op')
ms = {v: row['pose_iteration'][v]['median_ms'] for v in VARIANTS}
out.append({'torch_ops_over_op_by_op': round(ms['torch_ops'] / ms['op_by_op'], 3), 'torch_ops_over_fused': round(ms['torch_ops'] / ms['fused'], 3),
            'op_by_op_over_fused': round(ms['op_by_op'] / ms['fused'], 3)})
print(json.dumps(out[-1]), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        for ln in out:
            fh.write(json.dumps(ln) + '\n')
