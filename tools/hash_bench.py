"""Cost of the hash-grid sampler (csrc/hashgrid.hip, ops.hash_sample) beside what it replaces: ops.grid_sample of a
12-channel channels-last k0 at 160^3, forward plus backward, on the same positions, in the same process.

Positions come from real marches, in ray order (the backward's run merging depends on it; random points would flatter or
punish it wrongly): the kept samples of scenes.synthetic_scene(world=160) and the 8192 x 256 of scenes.roofline_scene.
Tables: L = 16, F = 2 and L = 8, F = 4, both 2^19 rows per hashed level, base 16, finest 512.  One process, every variant
warmed up, the variants alternating within a round, device-event timing, the median over rounds x reps and the spread (max -
min of the per-round medians) per variant:
  k0        ops.grid_sample forward, autograd backward (zero fill of the 197 MB gradient included: what a step pays)
  hash      ops.hash_sample forward, autograd backward (zero fill of the table's gradient included)
  bwd_*     dvgo_hash_bwd alone into a zero-filled buffer (the fill not timed): modes 1 and 3 at each run length, and mode 2
Added bytes per second of the backward: M * L * 8 * F * 4 B / t, to be read against the chip's 1.3 TB/s for contiguous
256-B atomic instructions and 0.08 TB/s for 64 lanes in 64 rows.
`--step`: one eager TrainStep of HashVoxGO on the synthetic scene beside DirectVoxGO(rgbnet_dim=12)'s eager step.
Prints one JSON line per case; `--out FILE` also writes them there.

  python tools/hash_bench.py [--reps 10] [--rounds 3] [--runs 1,2,4,8,16] [--step] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=10, help='timed calls per variant and round')
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--rays', type=int, default=8192)
ap.add_argument('--runs', default='1,2,4,8,16', help='comma list of run lengths for the backward A/B (modes 1 and 3)')
ap.add_argument('--step', action='store_true', help='also time one eager TrainStep against DirectVoxGO(rgbnet_dim=12)')
ap.add_argument('--out', default=None)
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from directvoxgo_amd import ops  # noqa: E402
from directvoxgo_amd.dvgo import DirectVoxGO  # noqa: E402
from directvoxgo_amd.fused import fused_march  # noqa: E402
from directvoxgo_amd.hashgrid import HASH_FINE_TRAIN, HashVoxGO, hash_levels  # noqa: E402
from directvoxgo_amd.scenes import roofline_scene, synthetic_scene  # noqa: E402
from directvoxgo_amd.train import FINE_TRAIN, TrainStep  # noqa: E402

assert torch.cuda.is_available(), 'hash_bench needs the GPU: a CPU run measures nothing'
RUNS = [int(v) for v in args.runs.split(',')]
TABLES = [dict(n_levels=16, n_feat=2), dict(n_levels=8, n_feat=4)]
WORLD = 160
BASE = dict(num_voxels=WORLD ** 3, num_voxels_base=WORLD ** 3, alpha_init=1e-2, fast_color_thres=1e-4)


def positions(sc):
    """The kept samples of the scene's rays, from the fused march, in ray order."""
    m = HashVoxGO(sc['xyz_min'], sc['xyz_max'], n_levels=2, log2_hashmap_size=4, **BASE).cuda()
    with torch.no_grad():
        m.density.copy_(sc['density']); m.mask_cache.mask.copy_(sc['mask'])
        cfg = m._march_cfg(sc['near'], sc['far'], sc['stepsize'])
        pts = fused_march(m.density, m.density.detach()[:, :0], sc['rays_o'], sc['rays_d'], cfg, positions=True)[3]
    return pts.contiguous(), m.xyz_min.clone(), m.xyz_max.clone()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    return r, (a, b)


def fwd_bwd(sample, param, gout, reps):
    ev_f, ev_b = [], []
    for _ in range(reps):
        param.grad = None
        out, e = timed(lambda: sample(param))
        ev_f.append(e)
        _, e = timed(lambda: out.backward(gout))
        ev_b.append(e)
        del out
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev_f], [a.elapsed_time(b) for a, b in ev_b]


def bwd_only(grad, gout, xyz, mn, mx, lv, run, mode, reps):
    ev = []
    for _ in range(reps):
        grad.zero_()
        ev.append(timed(lambda: ops.hash_bwd(gout, grad, xyz, mn, mx, lv, run=run, mode=mode))[1])
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def summary(rounds):
    """rounds: per round, the list of times -> median over everything, spread of the per-round medians"""
    meds = [float(np.median(r)) for r in rounds]
    return {'median_ms': round(float(np.median(np.concatenate(rounds))), 4), 'spread_ms': round(max(meds) - min(meds), 4)}


lines = []


def emit(row):
    lines.append(row)
    print(json.dumps(row), flush=True)


gen = torch.Generator(device='cuda').manual_seed(0)
scenes = {'synthetic_scene': synthetic_scene(world=WORLD, n_rays=args.rays, device='cuda'),
          'roofline_scene': roofline_scene(world=WORLD, n_rays=args.rays, device='cuda')}
for name, sc in scenes.items():
    xyz, mn, mx = positions(sc)
    M = xyz.shape[0]
    k0 = (torch.randn((1, 12, WORLD, WORLD, WORLD), generator=gen, device='cuda') * 0.3).contiguous(
        memory_format=torch.channels_last_3d).requires_grad_()
    gk = torch.randn((M, 12), generator=gen, device='cuda')
    k0_sample = lambda p: ops.grid_sample(p, xyz, mn, mx)          # noqa: E731
    for T in TABLES:
        L, Fc = T['n_levels'], T['n_feat']
        res, off = hash_levels(mn, mx, L, 16, 512, 19)
        lv = ops.HashLevels(res, off)
        table = torch.empty(lv.rows, Fc, device='cuda').uniform_(-1e-4, 1e-4, generator=gen).requires_grad_()
        gout = torch.randn((M, L * Fc), generator=gen, device='cuda')
        grad = torch.zeros(lv.rows, Fc, device='cuda')
        hash_sample = lambda p: ops.hash_sample(p, xyz, mn, mx, lv)          # noqa: E731
        variants = {'k0': (k0_sample, k0, gk), 'hash': (hash_sample, table, gout)}
        kernels = [(1, r) for r in RUNS] + [(3, r) for r in RUNS] + [(2, 0)]
        # same results first: every backward variant against mode 1, run 1 (relative to the largest gradient)
        ref = ops.hash_bwd(gout, torch.zeros_like(grad), xyz, mn, mx, lv, run=1, mode=1)
        agree = {}
        for mode, run in kernels:
            got = ops.hash_bwd(gout, torch.zeros_like(grad), xyz, mn, mx, lv, run=run, mode=mode)
            agree[f'mode{mode}_run{run}'] = float((got - ref).abs().max() / ref.abs().max())
        del ref, got
        for fn, p, g in variants.values():
            fwd_bwd(fn, p, g, 2)
        for mode, run in kernels:
            bwd_only(grad, gout, xyz, mn, mx, lv, run, mode, 2)
        TV = {v: {'fwd': [], 'bwd': []} for v in variants}
        TK = {k: [] for k in kernels}
        for _ in range(args.rounds):
            for v, (fn, p, g) in variants.items():
                f, b = fwd_bwd(fn, p, g, args.reps)
                TV[v]['fwd'].append(f); TV[v]['bwd'].append(b)
            for k in kernels:
                TK[k].append(bwd_only(grad, gout, xyz, mn, mx, lv, k[1], k[0], args.reps))
        added = M * L * 8 * Fc * 4
        row = {'scene': name, 'rays': args.rays, 'M': M, 'L': L, 'F': Fc, 'table_rows': lv.rows, 'dense_levels': lv.hashed.count(False),
               'table_MB': round(lv.rows * Fc * 4 / 2 ** 20, 1), 'max_rel_diff_to_mode1_run1': agree, 'added_bytes': added}
        for v in variants:
            row[v] = {'fwd': summary(TV[v]['fwd']), 'bwd': summary(TV[v]['bwd'])}
        row['bwd_kernel'] = {}
        for mode, run in kernels:
            s = summary(TK[(mode, run)])
            s['added_TBps'] = round(added / (s['median_ms'] * 1e-3) / 1e12, 4)
            row['bwd_kernel'][f'mode{mode}_run{run}'] = s
        row['hash_over_k0'] = {d: round(row['hash'][d]['median_ms'] / row['k0'][d]['median_ms'], 3) for d in ('fwd', 'bwd')}
        emit(row)
        del table, gout, grad, variants
        torch.cuda.empty_cache()
    del k0, gk
    torch.cuda.empty_cache()

if args.step:
    sc = scenes['synthetic_scene']
    rk = dict(near=sc['near'], far=sc['far'], bg=1, stepsize=sc['stepsize'])
    batch = (sc['rays_o'], sc['rays_d'], sc['viewdirs'], sc['target'])

    def step_times(model, cfg):
        with torch.no_grad():
            model.density.copy_(sc['density']); model.mask_cache.mask.copy_(sc['mask'])
        step = TrainStep(model, dict(cfg), rk)                       # never captured: the eager step
        for s in range(1, 4):
            step(*batch, global_step=s)
        rounds = []
        for _ in range(args.rounds):
            ev = [timed(lambda: step(*batch, global_step=10))[1] for _ in range(args.reps)]
            torch.cuda.synchronize()
            rounds.append([a.elapsed_time(b) for a, b in ev])
        return summary(rounds)

    torch.manual_seed(0)
    row = {'scene': 'synthetic_scene', 'rays': args.rays, 'eager_train_step_ms': {}}
    dv = DirectVoxGO(sc['xyz_min'], sc['xyz_max'], rgbnet_dim=12, **BASE).cuda()
    with torch.no_grad():
        dv.k0.copy_(sc['k0'])
    row['eager_train_step_ms']['DirectVoxGO_k0_12'] = step_times(dv, FINE_TRAIN)
    del dv
    torch.cuda.empty_cache()
    for T in TABLES:
        hv = HashVoxGO(sc['xyz_min'], sc['xyz_max'], **T, **BASE).cuda()
        row['eager_train_step_ms'][f"HashVoxGO_L{T['n_levels']}_F{T['n_feat']}"] = step_times(hv, HASH_FINE_TRAIN)
        del hv
        torch.cuda.empty_cache()
    emit(row)

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        for ln in lines:
            fh.write(json.dumps(ln) + '\n')
