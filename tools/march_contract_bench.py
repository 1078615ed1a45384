"""Speed of DirectContractedVoxGO's two forward paths: op by op (`fused_march=False`, the default) against the fused march
over contracted space (`fused_march=True`, csrc/march_contract.hip), the same model and state on the same device and rays.

Scene: the synthetic unbounded scene (scenes.unbounded_grids: a blob inside the unit box and an opaque textured shell behind
it) at --world^3 with a 12-channel feature grid and the HIP colour head, fast_color_thres 1e-4, stepsize 0.5, bg_len 0.2, rays
of cameras inside the foreground box (scenes.unbounded_cameras), the occupancy mask the model's own `_alpha_mask()`.
`fused_march` is a plain attribute, so ONE model serves both paths and they cannot drift apart; the training step runs with
learning rates of 1e-5 so that the scene stays what it is over the run.

Measured, one process, everything warmed up, the two paths alternating within a round, device-event timing, the median over
rounds x reps and the spread (max - min of the per-round medians):
  forward      model(...) under no_grad, --rays rays
  train_step   one TrainStep with weight_distortion = 0.01 (forward, losses, backward, optimizer)
  view         render_viewpoints of one --view x --view image (wall clock around a synchronise: it ends in a host copy)
  walk_only    fused_march_contract on an all-false occupancy mask: the ray setup, the geometry and the thinning walk of every
               chunk of every ray, no density read, no record (with the gather and the positions launches on zero samples)
and, counted: table steps per ray, the op-by-op path's occupied samples, the march's records and the kept samples.
Prints one JSON line per measurement and a last line with the ratios; `--out FILE` also writes them there.

  python tools/march_contract_bench.py [--world 160] [--reps 10] [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=10, help='timed calls per path and round')
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--rays', type=int, default=8192)
ap.add_argument('--world', type=int, default=160)
ap.add_argument('--view', type=int, default=800, help='side of the rendered view (0: skip)')
ap.add_argument('--out', default=None)
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from directvoxgo_amd import _lib as L  # noqa: E402
from directvoxgo_amd import fused as F  # noqa: E402
from directvoxgo_amd import scenes  # noqa: E402
from directvoxgo_amd.dcvgo import DirectContractedVoxGO  # noqa: E402
from directvoxgo_amd.render import render_viewpoints  # noqa: E402
from directvoxgo_amd.train import TrainStep  # noqa: E402

assert torch.cuda.is_available(), 'march_contract_bench needs the GPU: a CPU run measures nothing'
PATHS = ('op_by_op', 'fused')
RK = dict(near=0.0, far=1e4, stepsize=0.5, bg=0.5)
CFG = dict(N_iters=1000, N_rand=args.rays, lrate_density=1e-5, lrate_k0=1e-5, lrate_rgbnet=1e-5, lrate_decay=20, pervoxel_lr=False,
           weight_main=1.0, weight_entropy_last=0.001, weight_rgbper=0.01, tv_every=1, tv_after=0, tv_before=0, tv_dense_before=0,
           weight_tv_density=0.0, weight_tv_k0=0.0, pg_scale=[], skip_zero_grad_fields=['density', 'k0'], weight_distortion=0.01)

gen = torch.Generator().manual_seed(0)
W = args.world
model = DirectContractedVoxGO([-1, -1, -1], [1, 1, 1], num_voxels=W ** 3, num_voxels_base=W ** 3, alpha_init=1e-2,
                              fast_color_thres=1e-4, rgbnet_dim=12, rgbnet_direct=True).cuda()
density, _ = scenes.unbounded_grids(W, 0.2, gen)
with torch.no_grad():
    model.density.copy_(density.cuda())
    model.k0.copy_((torch.randn(model.k0.shape, generator=gen) * 0.3).cuda())
    model._set_mask_cache(model._alpha_mask())
del density
poses = scenes.unbounded_cameras(16, gen)
cams = [scenes.camera_rays(64, 64, 48.0, c2w) for c2w in poses]
pick = torch.randint(16 * 64 * 64, (args.rays,), generator=gen)
ro, rd, vd = (torch.cat([r[i] for r in cams])[pick].cuda().contiguous() for i in range(3))
target = torch.rand((args.rays, 3), generator=gen).cuda()
rays = (ro, rd, vd)


def on(path):
    model.fused_march = path == 'fused'


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def summary(rounds):
    meds = [float(np.median(r)) for r in rounds]
    return {'median_ms': round(float(np.median(np.concatenate(rounds))), 4), 'spread_ms': round(max(meds) - min(meds), 4)}


def alternate(fns, warm=3):
    """{path: callable} -> {path: summary}: warm-up, then rounds in which the paths take turns"""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    T = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            ev = [timed(fn) for _ in range(args.reps)]
            torch.cuda.synchronize()
            T[k].append([a.elapsed_time(b) for a, b in ev])
    return {k: summary(v) for k, v in T.items()}


out = [{'reps': args.reps, 'rounds': args.rounds, 'world': W, 'rays': args.rays, 'stepsize': RK['stepsize'], 'bg_len': model.bg_len}]
print(json.dumps(out[0]), flush=True)

res = {}
with torch.no_grad():
    for k in PATHS:
        on(k)
        res[k] = model(*rays, render_depth=True, **RK)
    occupied = int(model.sample_ray(ro, rd, RK['stepsize'])[0].shape[0])
    cfg = model._march_contract_cfg(RK['stepsize'], model.density.device)
    seen, orig = [], L.call
    L.call = lambda name, *a: (seen.append((name, a)), orig(name, *a))[1]
    try:
        F.fused_march_contract(model.density, ro, rd, cfg)
    finally:
        L.call = orig
    n2 = next(a for n, a in seen if n == 'dvgo_march_contract_density')[-4]                # include/dvgo_hip.h: (..., rec2, n2, n3, last, stream)
    records = int(n2.sum())
a, b = res['op_by_op'], res['fused']
same = {k: bool(torch.equal(a[k], b[k])) for k in a if k != 'n_max'}
out.append({'paths_agree_bit_for_bit': same})
print(json.dumps(out[-1]), flush=True)
out.append({'table_steps_per_ray': a['n_max'], 'chunks_per_ray': -(-a['n_max'] // 64), 'occupied_samples_op_by_op': occupied,
            'records_fused': records, 'kept_samples': int(a['ray_id'].shape[0]), 'rays_that_stop': int((a['alphainv_last'] < 1e-3).sum())})
print(json.dumps(out[-1]), flush=True)


def fwd(k):
    def run():
        on(k)
        with torch.no_grad():
            model(*rays, **RK)
    return run


row = {'forward': alternate({k: fwd(k) for k in PATHS})}
out.append(row)
print(json.dumps(row), flush=True)

# the thinning walk alone: the march on an all-false mask visits every chunk of every ray and skips each of them
off = F.ContractMarchConfig(model.scene_center, model.scene_radius, cfg.t_tab, model.bg_len, model.contracted_norm, cfg.thin_thres,
                            model.xyz_min, model.xyz_max, cfg.act_shift, cfg.interval, cfg.thres, mask=torch.zeros_like(cfg.mask),
                            xyz2ijk_scale=model.mask_cache.xyz2ijk_scale, xyz2ijk_shift=model.mask_cache.xyz2ijk_shift)


def walk():
    with torch.no_grad():
        F.fused_march_contract(model.density, ro, rd, off)


def march():
    with torch.no_grad():
        F.fused_march_contract(model.density, ro, rd, cfg)


row = {'walk_only': alternate({'all_false_mask': walk, 'scene_mask': march})}
out.append(row)
print(json.dumps(row), flush=True)

step = TrainStep(model, CFG, RK)
it = [0]


def train(k):
    def run():
        on(k)
        it[0] += 1
        step(ro, rd, vd, target, global_step=it[0])
    return run


row = {'train_step': alternate({k: train(k) for k in PATHS})}
out.append(row)
print(json.dumps(row), flush=True)

if args.view > 0:
    H = Wv = args.view
    Kmat = np.array([[0.75 * Wv, 0, 0.5 * Wv], [0, 0.75 * H, 0.5 * H], [0, 0, 1]], np.float32)
    pose = poses[0].numpy()
    T = {k: [] for k in PATHS}
    for k in PATHS:
        on(k)
        render_viewpoints(model, [pose], [(H, Wv)], [Kmat], False, RK)            # warm-up
    for _ in range(args.rounds):
        for k in PATHS:
            on(k)
            ts = []
            for _ in range(max(1, args.reps // 3)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                render_viewpoints(model, [pose], [(H, Wv)], [Kmat], False, RK)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            T[k].append(ts)
    row = {'view': {'side': args.view, **{k: summary(v) for k, v in T.items()}}}
    out.append(row)
    print(json.dumps(row), flush=True)

on('op_by_op')
ratios = {}
for row in out:
    for what in ('forward', 'train_step', 'view'):
        if what in row:
            ratios[what + '_op_by_op_over_fused'] = round(row[what]['op_by_op']['median_ms'] / row[what]['fused']['median_ms'], 3)
out.append(ratios)
print(json.dumps(ratios), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        for ln in out:
            fh.write(json.dumps(ln) + '\n')
