"""Speed of the positional-encoding colour head (csrc/shade_pe.hip) on its workload: the lego-like 160^3 scene
(scenes.synthetic_scene) with posbase_pe = 10 and the 128-wide rgbnet_direct head, in one process, warmed up, the two
variants alternating, device-event timing:
  * the training step's forward + loss + backward in 8192-ray batches, new head vs `model.fused_shade = False` (the torch
    head on the same fused march);
  * one 800x800 view through render_viewpoints, both heads.
Prints one JSON line.  With `--kernel-stats CSV` (a `rocprofv3 --kernel-trace --stats` run of this tool) it prints, instead
and without touching the GPU, each head kernel's mean time against its fp32 matrix-core floor at 157.3 TFLOP/s, for the mean
sample count the trace run printed (`--samples`).

  python tools/posenc_bench.py [--steps 20] [--views 2]
  rocprofv3 --kernel-trace --stats -d DIR -o pe -- python tools/posenc_bench.py --steps 20 --views 0
  python tools/posenc_bench.py --kernel-stats DIR/.../pe_kernel_stats.csv --samples M
"""
import argparse
import csv
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 157.3e12
WIDTH, P, E = 128, 10, 27
D_IN = 3 + 6 * P + E
# FLOP per sample of each kernel's matrix work (the dense contractions; biases, ReLU, sigmoid and sin/cos not counted)
FLOP = {'pe_fwd_kernel': 2 * (D_IN * WIDTH + WIDTH * WIDTH + WIDTH * 3),
        'pe_bwd_kernel': 2 * (WIDTH * WIDTH + WIDTH * 3),
        'pe_wgrad_kernel': 2 * (D_IN * WIDTH + WIDTH * WIDTH + WIDTH * 3)}

ap = argparse.ArgumentParser()
ap.add_argument('--world', type=int, default=160)
ap.add_argument('--rays', type=int, default=8192)
ap.add_argument('--steps', type=int, default=20, help='timed training steps per variant and round')
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--views', type=int, default=2, help='timed 800x800 views per variant and round (0: none)')
ap.add_argument('--kernel-stats', default=None)
ap.add_argument('--samples', type=float, default=None, help='mean samples per training batch (with --kernel-stats)')
args = ap.parse_args()


def kernel_table(path, samples):
    rows = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name = r.get('Name') or r.get('KernelName') or ''
            for k in FLOP:
                if k in name:
                    rows[k] = (int(r['Calls']), float(r['AverageNs']) / 1e3)
    out = {}
    for k, (calls, avg_us) in sorted(rows.items()):
        floor_us = samples * FLOP[k] / PEAK * 1e6
        out[k] = {'calls': calls, 'mean_us': round(avg_us, 1), 'floor_us': round(floor_us, 1),
                  'floor_share': round(floor_us / avg_us, 3)}
    return out


if args.kernel_stats:
    print(json.dumps({'samples': args.samples, 'kernels': kernel_table(args.kernel_stats, args.samples)}))
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from directvoxgo_amd.dvgo import DirectVoxGO  # noqa: E402
from directvoxgo_amd.render import render_viewpoints  # noqa: E402
from directvoxgo_amd.scenes import lego_like_rays, pose_spherical, synthetic_scene  # noqa: E402
from directvoxgo_amd.train import FINE_TRAIN, fused_render_loss  # noqa: E402

sc = synthetic_scene(world=args.world, n_rays=8, device='cuda')
m = DirectVoxGO(sc['xyz_min'], sc['xyz_max'], num_voxels=args.world ** 3, num_voxels_base=args.world ** 3, alpha_init=1e-2,
                fast_color_thres=1e-4, rgbnet_dim=12, rgbnet_width=WIDTH, rgbnet_direct=True, posbase_pe=P)
torch.manual_seed(0)
for p in m.rgbnet.parameters():
    torch.nn.init.normal_(p, std=0.1)
m = m.cuda()
with torch.no_grad():
    m.density.copy_(sc['density']); m.k0.copy_(sc['k0']); m.mask_cache.mask.copy_(sc['mask'])
gen = torch.Generator().manual_seed(1)
batches = []
for _ in range(args.steps):
    ro, rd, vd = lego_like_rays(args.rays, gen)
    batches.append((ro.cuda(), rd.cuda(), vd.cuda(), torch.rand((args.rays, 3), generator=gen).cuda()))
rk = dict(near=sc['near'], far=sc['far'], bg=1, stepsize=0.5)
cfg = dict(FINE_TRAIN)


def train_steps():
    """mean ms of forward + loss + backward per batch, and the mean sample count"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in batches]
    n = 0
    for (ro, rd, vd, tgt), (a, b) in zip(batches, ev):
        m.zero_grad(set_to_none=True)
        a.record()
        res = m(ro, rd, vd, global_step=1, **rk)
        fused_render_loss(res, tgt, args.rays, cfg).backward()
        b.record()
        n += res['weights'].shape[0]
    torch.cuda.synchronize()
    return float(np.mean([a.elapsed_time(b) for a, b in ev])), n / len(batches)


H = W = 800
K = np.array([[1111.11, 0, 0.5 * W], [0, 1111.11, 0.5 * H], [0, 0, 1]], np.float32)
poses = [pose_spherical(40.0 * i - 60, -30.0, 4.0).numpy() for i in range(max(args.views, 1))]


def render():
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    render_viewpoints(m, poses[:args.views], [(H, W)] * args.views, [K] * args.views, False, dict(rk, inverse_y=False), chunk=8192)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / args.views


res = {'hip': {'step_ms': [], 'view_ms': []}, 'torch': {'step_ms': [], 'view_ms': []}}
for variant in ('hip', 'torch'):                       # warm-up of both
    m.fused_shade = variant == 'hip'
    train_steps()
    if args.views:
        render()
samples = None
for _ in range(args.rounds):
    for variant in ('hip', 'torch'):
        m.fused_shade = variant == 'hip'
        t, samples = train_steps()
        res[variant]['step_ms'].append(round(t, 3))
        if args.views:
            res[variant]['view_ms'].append(round(render(), 2))
out = {'scene': f'{args.world}^3 lego-like, posbase_pe={P}, width {WIDTH}, {args.rays}-ray batches', 'samples_per_batch': samples}
for v in res:
    out[v] = {'step_ms_median': float(np.median(res[v]['step_ms'])), 'step_ms': res[v]['step_ms']}
    if args.views:
        out[v].update(view_ms_median=float(np.median(res[v]['view_ms'])), view_ms=res[v]['view_ms'])
out['step_speedup'] = round(out['torch']['step_ms_median'] / out['hip']['step_ms_median'], 3)
if args.views:
    out['view_speedup'] = round(out['torch']['view_ms_median'] / out['hip']['view_ms_median'], 3)
print(json.dumps(out))
