"""Speed of the tri-plane sampler (csrc/triplane.hip, ops.triplane_sample) against what a user runs without it: three
F.grid_sample calls plus cat or add, with the autograd backward (lib/tri_dvgo.py:456-469), on the same device and inputs.

Positions: the kept samples of the roofline scene (scenes.roofline_scene: 8192 rays x 256 samples = 2 097 152), from the
fused march.  Cases: planes 160^2 and 200^2, C in {12, 32}, 'concat' and 'sum'.  One process, every shape warmed up, the
variants alternating within a round, device-event timing, the median over rounds x reps and the spread (max - min of
the per-round medians) reported per variant:
  torch    channel-first planes [1,C,H,W] (the reference's layout), grid_sample x 3 + cat / add; backward by autograd
  hip      ops.triplane_sample on the same channel-first planes (the op hands the kernels channels-last copies)
  hip_cl   ops.triplane_sample on channels-last planes (TriPlaneVoxGO's own storage)
  bwd_runN the backward kernel alone (ops.triplane_bwd into zero-filled channels-last buffers, the zero fill not timed) with a
           lane merging runs of N consecutive samples before its atomics; N = 1 is no merging
Forward bytes: the algorithmic traffic M * (4 * width + 12) (output write + position read) over the hip_cl forward time.
Prints one JSON line per case and a last line with the verdict; `--out FILE` also writes them there.

  python tools/triplane_bench.py [--reps 10] [--rounds 3] [--out FILE]
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
ap.add_argument('--runs', default='1,2,4,8', help='comma list of run lengths for the backward A/B')
ap.add_argument('--sizes', default='160,200')
ap.add_argument('--channels', default='12,32')
ap.add_argument('--out', default=None)
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from directvoxgo_amd import ops  # noqa: E402
from directvoxgo_amd.fused import fused_march  # noqa: E402
from directvoxgo_amd.scenes import roofline_scene  # noqa: E402
from directvoxgo_amd.triplane import TriPlaneVoxGO  # noqa: E402

assert torch.cuda.is_available(), 'triplane_bench needs the GPU: a CPU run measures nothing'
KEYS = ('xy', 'yz', 'zx')
PAIRS = {'xy': [0, 1], 'yz': [1, 2], 'zx': [2, 0]}
RUNS = [int(v) for v in args.runs.split(',')]


def positions():
    sc = roofline_scene(world=160, n_rays=args.rays, device='cuda')
    m = TriPlaneVoxGO(sc['xyz_min'], sc['xyz_max'], num_voxels=160 ** 3, num_voxels_base=160 ** 3, alpha_init=1e-2,
                      fast_color_thres=1e-4, rgbnet_dim=4, plane_size=(8, 8)).cuda()
    with torch.no_grad():
        m.density.copy_(sc['density']); m.mask_cache.mask.copy_(sc['mask'])
        cfg = m._march_cfg(sc['near'], sc['far'], sc['stepsize'])
        pts = fused_march(m.density, m.density.detach()[:, :0], sc['rays_o'], sc['rays_d'], cfg, positions=True)[3]
    return pts.contiguous(), m.xyz_min.clone(), m.xyz_max.clone()


def torch_sample(planes, xyz, mn, mx, agg):
    """lib/tri_dvgo.py:456-469, expression for expression"""
    x = xyz.reshape(1, 1, -1, 3)
    ind_norm = ((x - mn) / (mx - mn)).flip((-1,)) * 2 - 1
    f = [F.grid_sample(planes[k], ind_norm[..., PAIRS[k]], mode='bilinear', align_corners=True)[0, :, 0, :].T for k in KEYS]
    return torch.cat(f, dim=-1) if agg == 'concat' else f[0] + f[1] + f[2]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    return r, (a, b)


def fwd_bwd(sample, planes, xyz, mn, mx, agg, gout, reps):
    ev_f, ev_b = [], []
    for _ in range(reps):
        for p in planes.values():
            p.grad = None
        out, e = timed(lambda: sample(planes, xyz, mn, mx, agg))
        ev_f.append(e)
        _, e = timed(lambda: out.backward(gout))
        ev_b.append(e)
        del out
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev_f], [a.elapsed_time(b) for a, b in ev_b]


def bwd_only(grads, xyz, mn, mx, agg, gout, run, reps):
    ev = []
    for _ in range(reps):
        for g in grads.values():
            g.zero_()
        ev.append(timed(lambda: ops.triplane_bwd(gout, grads, xyz, mn, mx, agg, run=run))[1])
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def summary(rounds):
    """rounds: per round, the list of times -> median over everything, spread of the per-round medians"""
    meds = [float(np.median(r)) for r in rounds]
    return {'median_ms': round(float(np.median(np.concatenate(rounds))), 4), 'spread_ms': round(max(meds) - min(meds), 4)}


xyz, mn, mx = positions()
M = xyz.shape[0]
lines = [{'positions': M, 'source': f'roofline scene 160^3, {args.rays} rays', 'reps': args.reps, 'rounds': args.rounds}]
print(json.dumps(lines[0]), flush=True)
gen = torch.Generator(device='cuda').manual_seed(0)
verdict = []
for S in [int(v) for v in args.sizes.split(',')]:
    for C in [int(v) for v in args.channels.split(',')]:
        for agg in ('concat', 'sum'):
            width = 3 * C if agg == 'concat' else C
            base = {k: torch.randn((1, C, S, S), generator=gen, device='cuda') * 0.3 for k in KEYS}
            gout = torch.randn((M, width), generator=gen, device='cuda')
            variants = {
                'torch': (torch_sample, {k: v.clone().requires_grad_() for k, v in base.items()}),
                'hip': (ops.triplane_sample, {k: v.clone().requires_grad_() for k, v in base.items()}),
                'hip_cl': (ops.triplane_sample, {k: v.clone().contiguous(memory_format=torch.channels_last).requires_grad_()
                                                 for k, v in base.items()}),
            }
            grads = {k: torch.zeros_like(v, memory_format=torch.channels_last) for k, v in base.items()}
            # same results first (section 6 of the measuring guide), then the warm-up of every variant
            with torch.no_grad():
                ref = torch_sample(base, xyz, mn, mx, agg)
                got = ops.triplane_sample(base, xyz, mn, mx, agg)
                max_diff = float((ref - got).abs().max())
                del ref, got
            for fn, pl in variants.values():
                fwd_bwd(fn, pl, xyz, mn, mx, agg, gout, 2)
            g_ref, g_hip = variants['torch'][1]['xy'].grad, variants['hip'][1]['xy'].grad
            grad_diff = float((g_ref - g_hip).abs().max() / g_ref.abs().max())
            for run in RUNS:
                bwd_only(grads, xyz, mn, mx, agg, gout, run, 2)
            T = {v: {'fwd': [], 'bwd': []} for v in variants}
            TR = {run: [] for run in RUNS}
            for _ in range(args.rounds):
                for v, (fn, pl) in variants.items():
                    f, b = fwd_bwd(fn, pl, xyz, mn, mx, agg, gout, args.reps)
                    T[v]['fwd'].append(f); T[v]['bwd'].append(b)
                for run in RUNS:
                    TR[run].append(bwd_only(grads, xyz, mn, mx, agg, gout, run, args.reps))
            row = {'plane': S, 'C': C, 'aggregation': agg, 'max_abs_diff_fwd': max_diff, 'rel_diff_grad_xy': grad_diff}
            for v in variants:
                row[v] = {'fwd': summary(T[v]['fwd']), 'bwd': summary(T[v]['bwd'])}
            row['bwd_kernel_by_run'] = {str(run): summary(TR[run]) for run in RUNS}
            fwd_bytes = M * (4 * width + 12)
            row['fwd_algorithmic_bytes'] = fwd_bytes
            row['hip_cl_fwd_TBps'] = round(fwd_bytes / (row['hip_cl']['fwd']['median_ms'] * 1e-3) / 1e12, 3)
            row['atomic_bytes'] = M * 12 * C * 4
            for v in ('hip', 'hip_cl'):
                for d in ('fwd', 'bwd'):
                    spread = max(row[v][d]['spread_ms'], row['torch'][d]['spread_ms'])
                    ok = row[v][d]['median_ms'] <= row['torch'][d]['median_ms'] + spread
                    verdict.append(ok)
                    row[f'{v}_{d}_no_slower_than_torch'] = ok
            lines.append(row)
            print(json.dumps(row), flush=True)
            del variants, grads, base, gout
            torch.cuda.empty_cache()
lines.append({'every_case_meets_the_bar': all(verdict), 'cases': len(verdict)})
print(json.dumps(lines[-1]), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        for ln in lines:
            fh.write(json.dumps(ln) + '\n')
