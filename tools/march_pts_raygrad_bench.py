"""What a camera-pose iteration costs on the fused march for HashVoxGO, VMTriPlaneVoxGO and TensoRFVoxGO (raygrad='fused':
csrc/march_raygrad.hip, dvgo_march_ray_bwd_pts / dvgo_march_vm_ray_bwd) beside the same iteration op by op
(DirectVoxGO._forward_raygrad), at the sizes of tools/hash_raygrad_bench.py --pose and tools/vm_raygrad_bench.py --pose:
scenes.synthetic_scene at 160^3, --rays random pixels of 24 views of 128 x 128; the hash table L = 16, F = 2; planes and lines
R = 16 following the grid; TensoRFVoxGO(fused_march=True) on a density of separable bumps.

Per model, one model object; the two paths differ in the instance's `fused_raygrad` alone (False: op by op).  One process, every
variant warmed up, the variants alternating within a round, device events around each call, the median over rounds x reps and
the spread (max - min of the per-round medians):
  frozen_op_by_op / frozen_fused   one pose iteration, the model frozen: CameraRefiner.rays -> model -> train.render_loss ->
                                   backward into delta -> Adam on delta (what pose.refine_poses does per iteration)
  joint_op_by_op                   poses and model: the same plus the model's eager optimiser (refine_poses(train_model=True))
  joint_fused                      poses and model through a train.TrainStep (refine_poses(train_model=True, fused=True))
  kernels                          inside the frozen fused iterations, events around the new entry and around the forward launch
                                   that wrote its records (_lib.profile_start): mean ms per launch
The learning rates of the joint runs are scaled by 1e-6, so the scene stays what it is over the run.  The ray gradients of both
paths are compared first (largest difference over the largest gradient: a report).
Prints one JSON line per model; `--out FILE` also writes them there.

  python tools/march_pts_raygrad_bench.py [--reps 10] [--rounds 3] [--rays 8192] [--out FILE]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=10, help='timed calls per variant and round')
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--rays', type=int, default=8192)
ap.add_argument('--out', default=None)
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from directvoxgo_amd import _lib as L  # noqa: E402
from directvoxgo_amd.hashgrid import HASH_FINE_TRAIN, HashVoxGO  # noqa: E402
from directvoxgo_amd.ops import PLANE_KEYS  # noqa: E402
from directvoxgo_amd.pose import CameraRefiner  # noqa: E402
from directvoxgo_amd.scenes import pose_spherical, synthetic_scene  # noqa: E402
from directvoxgo_amd.tensorf import TENSORF_FINE_TRAIN, TensoRFVoxGO  # noqa: E402
from directvoxgo_amd.train import TrainStep, create_optimizer_or_freeze_model, render_loss  # noqa: E402
from directvoxgo_amd.vm import VM_FINE_TRAIN, VMTriPlaneVoxGO  # noqa: E402

assert torch.cuda.is_available(), 'march_pts_raygrad_bench needs the GPU: a CPU run measures nothing'
WORLD, R = 160, 16
BASE = dict(num_voxels=WORLD ** 3, num_voxels_base=WORLD ** 3, alpha_init=1e-2, fast_color_thres=1e-4)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def series(fn, reps):
    ev = [timed(fn) for _ in range(reps)]
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def summary(rounds):
    meds = [float(np.median(r)) for r in rounds]
    return {'median_ms': round(float(np.median(np.concatenate(rounds))), 4), 'spread_ms': round(max(meds) - min(meds), 4)}


def bump(k, centre, width=0.45):
    return torch.exp(-((torch.linspace(-1, 1, k, device='cuda') - centre) / width) ** 2)


def build(name, sc):
    torch.manual_seed(0)
    if name == 'HashVoxGO':
        m = HashVoxGO(sc['xyz_min'], sc['xyz_max'], raygrad='fused', n_levels=16, n_feat=2, **BASE).cuda()
        cfg, entry, fwd = HASH_FINE_TRAIN, 'dvgo_march_ray_bwd_pts', 'dvgo_march_density'
    elif name == 'VMTriPlaneVoxGO':
        m = VMTriPlaneVoxGO(sc['xyz_min'], sc['xyz_max'], raygrad='fused', n_comp=R, **BASE).cuda()
        cfg, entry, fwd = VM_FINE_TRAIN, 'dvgo_march_ray_bwd_pts', 'dvgo_march_density'
    else:
        m = TensoRFVoxGO(sc['xyz_min'], sc['xyz_max'], raygrad='fused', n_comp=R, density_n_comp=R, fused_march=True, **BASE).cuda()
        cfg, entry, fwd = TENSORF_FINE_TRAIN, 'dvgo_march_vm_ray_bwd', 'dvgo_march_vm_density'
    with torch.no_grad():
        if name == 'TensoRFVoxGO':               # separable bumps plus a negative constant, as in tests/vm_render_oracle.py
            for i, k in enumerate(PLANE_KEYS):
                p, ln = m.density_planes[k], m.density_lines[k]
                p.mul_(0.5); ln.mul_(0.5)
                c = 0.25 * (i - 1)
                p[0, 0] = 3.0 * bump(p.shape[2], c)[:, None] * bump(p.shape[3], -c)[None, :]
                ln[0, 0, :, 0] = 3.0 * bump(ln.shape[2], 0.1 * i)
                p[0, 1] = 1.0
                ln[0, 1] = -1.0
            m.mask_cache.mask.fill_(True)
        else:
            m.density.copy_(sc['density']); m.mask_cache.mask.copy_(sc['mask'])
        if name == 'HashVoxGO':
            m.hash_table.normal_(0, 0.5)
        else:
            for q in list(m.planes.values()) + list(m.lines.values()):
                q.normal_(0, 0.5)
    cfg = {k: (v * 1e-6 if k.startswith('lrate_') and k != 'lrate_decay' else v) for k, v in cfg.items()}
    return m, dict(cfg, weight_entropy_last=0.0, weight_rgbper=0.0), entry, fwd


lines = []
sc = synthetic_scene(world=WORLD, n_rays=args.rays, device='cuda')
rk = dict(near=sc['near'], far=sc['far'], bg=1, stepsize=sc['stepsize'])
n, S = 24, 128
poses = torch.stack([pose_spherical(15.0 * i, -30.0, 4.0)[:3, :4] for i in range(n)])
K = np.array([[1.39 * S, 0, 0.5 * S], [0, 1.39 * S, 0.5 * S], [0, 0, 1]], np.float32)       # lego's field of view
refiner = CameraRefiner(poses, np.array([[S, S]] * n), np.stack([K] * n)).cuda()
opt = torch.optim.Adam([refiner.delta], lr=1e-9)                 # (the poses stay what they are over the run)
cpu = torch.Generator().manual_seed(7)
view = torch.randint(n, (args.rays,), generator=cpu).cuda()
pix_i = torch.randint(S, (args.rays,), generator=cpu).cuda()
pix_j = torch.randint(S, (args.rays,), generator=cpu).cuda()
target = torch.rand((args.rays, 3), generator=cpu).cuda()

for name in ('HashVoxGO', 'VMTriPlaneVoxGO', 'TensoRFVoxGO'):
    model, cfg, entry, fwd = build(name, sc)
    kept = []

    def frozen(fused):
        model.fused_raygrad = fused
        rays_o, rays_d, viewdirs = refiner.rays(view, pix_i, pix_j)
        out = model(rays_o, rays_d, viewdirs, global_step=None, **rk)
        loss = render_loss(out, target, args.rays, cfg)
        opt.zero_grad(set_to_none=True)
        loss.backward(inputs=[refiner.delta])
        opt.step()
        kept.append(int(out['ray_id'].shape[0]))

    # the two paths give the same gradient up to rounding
    grads = []
    for fused in (False, True):
        frozen(fused)
        grads.append(refiner.delta.grad.detach().clone())
    diff = float((grads[0] - grads[1]).abs().max() / grads[0].abs().max())
    opt_model = create_optimizer_or_freeze_model(model, cfg, 0)
    step = TrainStep(model, cfg, rk)
    it = [0]

    def joint_op_by_op():
        model.fused_raygrad = False
        rays_o, rays_d, viewdirs = refiner.rays(view, pix_i, pix_j)
        out = model(rays_o, rays_d, viewdirs, global_step=None, **rk)
        loss = render_loss(out, target, args.rays, cfg)
        opt.zero_grad(set_to_none=True)
        opt_model.zero_grad(set_to_none=True)
        loss.backward()
        opt_model.step()
        opt.step()

    def joint_fused():
        model.fused_raygrad = True
        it[0] += 1
        rays_o, rays_d, viewdirs = refiner.rays(view, pix_i, pix_j)
        opt.zero_grad(set_to_none=True)
        step(rays_o, rays_d, viewdirs, target, it[0])
        opt.step()

    def set_frozen(flag):
        for q in model.parameters():
            q.requires_grad_(not flag)

    variants = {'frozen_op_by_op': (True, lambda: frozen(False)), 'frozen_fused': (True, lambda: frozen(True)),
                'joint_op_by_op': (False, joint_op_by_op), 'joint_fused': (False, joint_fused)}
    for is_frozen, fn in variants.values():
        set_frozen(is_frozen)
        series(fn, 3)
    T = {v: [] for v in variants}
    for _ in range(args.rounds):
        for v, (is_frozen, fn) in variants.items():
            set_frozen(is_frozen)
            T[v].append(series(fn, args.reps))
    set_frozen(True)
    L.profile_start([entry, fwd])
    for _ in range(args.reps * args.rounds):
        frozen(True)
    prof = L.profile_stop()
    row = {'model': name, 'scene': 'synthetic_scene', 'world': WORLD, 'rays': args.rays, 'views': n, 'side': S, 'reps': args.reps,
           'rounds': args.rounds, 'kept_samples': kept[-1], 'delta_grad_max_diff_over_max': diff}
    for v in variants:
        row[v] = summary(T[v])
    row['frozen_op_by_op_over_fused'] = round(row['frozen_op_by_op']['median_ms'] / row['frozen_fused']['median_ms'], 3)
    row['joint_op_by_op_over_fused'] = round(row['joint_op_by_op']['median_ms'] / row['joint_fused']['median_ms'], 3)
    row['kernels'] = {k: {'launches': c, 'mean_ms': round(ms / max(c, 1), 4)} for k, (c, ms) in prof.items()}
    lines.append(row)
    print(json.dumps(row), flush=True)
    del model, step, opt_model
    torch.cuda.empty_cache()

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        for ln in lines:
            fh.write(json.dumps(ln) + '\n')
