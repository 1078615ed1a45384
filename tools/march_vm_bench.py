"""Speed of TensoRFVoxGO's two render paths: op by op (`fused_march=False`) against the fused march over the decomposed
density (`fused_march=True`, csrc/march_vm.hip), the same model and state on the same device and rays.

Scene: 160^3, density_n_comp = 16, n_comp = 16, rgbnet_dim 12, `scenes.lego_like_rays(8192)`.  The density is one the
decomposition represents exactly and that has a surface for rays to stop at: component 0 of plane and line xy hold a
separable Gaussian blob (raw density `--amp` at the centre, width `--sigma`), everything else is 0.01 * randn, and
density_offset = -9 keeps the space around the blob empty; the occupancy mask is the model's own `_alpha_mask()`.

Measured, one process, everything warmed up, the two paths alternating within a round, device-event timing, the median
over rounds x reps and the spread (max - min of the per-round medians):
  train_step   one TrainStep (forward, backward, optimizer)
  forward      model(...) under no_grad
  view         render_viewpoints of one 800 x 800 view (wall clock around a synchronise: it ends in a host copy)
and, counted, not timed: the samples the density is evaluated at per forward -- op by op every occupied step of every ray
(the M of its dvgo_vm_density_fwd launch); fused the occupied steps of the 64-step chunks a ray visits before it stops
(reconstructed on the host from the op-by-op sample list and the stop step of each ray) -- and the records and kept samples.
Prints one JSON line per measurement and a last line with the ratios; `--out FILE` also writes them there.

  python tools/march_vm_bench.py [--reps 10] [--rounds 3] [--out FILE]
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
ap.add_argument('--comp', type=int, default=16, help='density_n_comp')
ap.add_argument('--amp', type=float, default=20.0)
ap.add_argument('--sigma', type=float, default=0.6)
ap.add_argument('--view', type=int, default=800, help='side of the rendered view (0: skip)')
ap.add_argument('--out', default=None)
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from directvoxgo_amd import _lib as L  # noqa: E402
from directvoxgo_amd.checkpoint import model_kwargs_of  # noqa: E402
from directvoxgo_amd.render import render_viewpoints  # noqa: E402
from directvoxgo_amd.scenes import lego_like_rays, pose_spherical  # noqa: E402
from directvoxgo_amd.tensorf import TENSORF_FINE_TRAIN, TensoRFVoxGO  # noqa: E402
from directvoxgo_amd.train import TrainStep  # noqa: E402

assert torch.cuda.is_available(), 'march_vm_bench needs the GPU: a CPU run measures nothing'
PATHS = ('op_by_op', 'fused')
BOX = 1.5 * 1.05
RK = dict(near=2.0, far=6.0, bg=1, stepsize=0.5)


def make_models():
    torch.manual_seed(0)
    W = args.world
    m = TensoRFVoxGO([-BOX] * 3, [BOX] * 3, num_voxels=W ** 3, num_voxels_base=W ** 3, alpha_init=1e-2, fast_color_thres=1e-4,
                     n_comp=16, density_n_comp=args.comp, density_offset=-9.0, rgbnet_dim=12).cuda()
    with torch.no_grad():
        for p in list(m.density_planes.values()) + list(m.density_lines.values()):
            p.mul_(0.1)
        pl, ln = m.density_planes['xy'], m.density_lines['xy']
        ax = [torch.linspace(-BOX, BOX, n, device='cuda') for n in (pl.shape[2], pl.shape[3], ln.shape[2])]
        pl[0, 0] = args.amp * torch.exp(-(ax[0][:, None] ** 2 + ax[1][None, :] ** 2) / args.sigma ** 2)
        ln[0, 0, :, 0] = torch.exp(-ax[2] ** 2 / args.sigma ** 2)
        m._set_mask_cache(m._alpha_mask())
    f = TensoRFVoxGO(**{**model_kwargs_of({'model_kwargs': m.get_kwargs()}), 'fused_march': True}).cuda()
    f.load_state_dict(m.state_dict())
    f._set_mask_cache(m.mask_cache.mask.clone())
    return {'op_by_op': m, 'fused': f}


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


def counts(models, rays):
    """samples the density is evaluated at, per path, and what comes out of the march"""
    m = models['op_by_op']
    seen, orig = [], L.call
    L.call = lambda name, *a: (seen.append((name, a)), orig(name, *a))[1]
    try:
        with torch.no_grad():
            res = m(*rays, **RK)
            models['fused'](*rays, **RK)
    finally:
        L.call = orig
    evaluated = [a[-3] for n, a in seen if n == 'dvgo_vm_density_fwd']            # (..., M, out, stream)
    assert len(evaluated) == 1
    a = next(a for n, a in seen if n == 'dvgo_march_vm_density')                  # include/dvgo_hip.h: the argument order
    stride, N, rec2, n2, last = a[3], a[4], a[-9], a[-8], a[-6]
    with torch.no_grad():
        # the chunk a ray stops in: that of its last record, when the transmittance fell below 1e-3 there
        steps = rec2[:N * stride].view(N, stride, 4)[:, :, 0].contiguous().view(torch.int32).long() & 0x7fffffff
        last_step = steps.gather(1, (n2.long() - 1).clamp(min=0)[:, None])[:, 0]
        stopped = (last < 1e-3) & (n2 > 0)
        end = torch.where(stopped, (last_step // 64 + 1) * 64, torch.full_like(last_step, 1 << 40))
        pts, ray_id, step_id = m.sample_ray(rays_o=rays[0], rays_d=rays[1], **RK)
        occ = m.mask_cache(pts)
        ray_id, step_id = ray_id[occ], step_id[occ]
        assert ray_id.shape[0] == evaluated[0]
        fused_eval = int((step_id < end[ray_id]).sum())
    return {'rays': N, 'steps_in_box': int(pts.shape[0]), 'density_evaluated_op_by_op': int(evaluated[0]),
            'density_evaluated_fused': fused_eval, 'share_saved_by_the_early_stop': round(1 - fused_eval / max(evaluated[0], 1), 4),
            'rays_that_stop': int(stopped.sum()), 'records': int(n2.sum()), 'kept_samples': int(res['ray_id'].shape[0])}


out = [{'reps': args.reps, 'rounds': args.rounds, 'world': args.world, 'density_n_comp': args.comp, 'rays': args.rays,
        'amp': args.amp, 'sigma': args.sigma}]
print(json.dumps(out[0]), flush=True)
models = make_models()
gen = torch.Generator().manual_seed(777)
ro, rd, vd = (t.cuda() for t in lego_like_rays(args.rays, gen))
target = torch.rand((args.rays, 3), generator=gen).cuda()
rays = (ro, rd, vd)

with torch.no_grad():
    a, b = (models[k](*rays, render_depth=True, **RK) for k in PATHS)
same = {k: bool(torch.equal(a[k], b[k])) for k in ('ray_id', 'weights', 'raw_alpha', 'alphainv_last', 'raw_rgb', 'rgb_marched', 'depth')}
out.append({'paths_agree_bit_for_bit': same})
print(json.dumps(out[-1]), flush=True)
out.append(counts(models, rays))
print(json.dumps(out[-1]), flush=True)


def fwd(m):
    def run():
        with torch.no_grad():
            m(*rays, **RK)
    return run


row = {'forward': alternate({k: fwd(models[k]) for k in PATHS})}
out.append(row)
print(json.dumps(row), flush=True)

# the training step changes the parameters: each path trains a copy of its own from the same state
state = {k: v.detach().clone() for k, v in models['op_by_op'].state_dict().items()}
steps, it = {}, {k: 0 for k in PATHS}
for k in PATHS:
    steps[k] = TrainStep(models[k], dict(TENSORF_FINE_TRAIN), RK)


def train(k):
    def run():
        it[k] += 1
        steps[k](ro, rd, vd, target, global_step=it[k])
    return run


row = {'train_step': alternate({k: train(k) for k in PATHS})}
out.append(row)
print(json.dumps(row), flush=True)
for k in PATHS:
    models[k].load_state_dict(state)

if args.view > 0:
    H = W = args.view
    K = np.array([[1111.11 * W / 800, 0, 0.5 * W], [0, 1111.11 * H / 800, 0.5 * H], [0, 0, 1]], np.float32)
    pose = pose_spherical(30.0, -30.0, 4.0).numpy()
    rk = dict(RK, inverse_y=False)
    T = {k: [] for k in PATHS}
    for k in PATHS:
        render_viewpoints(models[k], [pose], [(H, W)], [K], False, rk)            # warm-up
    for _ in range(args.rounds):
        for k in PATHS:
            ts = []
            for _ in range(max(1, args.reps // 3)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                render_viewpoints(models[k], [pose], [(H, W)], [K], False, rk)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            T[k].append(ts)
    row = {'view': {'side': args.view, **{k: summary(v) for k, v in T.items()}}}
    out.append(row)
    print(json.dumps(row), flush=True)

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
