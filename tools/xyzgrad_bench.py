"""Speed of the position gradient of the trilinear sample (csrc/grid_sample_xyz.hip: dvgo_grid_sample_bwd_xyz) against
what a user has without it: torch's own F.grid_sample backward with the sample grid requiring grad (and the volume not),
on the same device, volume values and positions.

Cases (what pose refinement runs on every kept sample of every step):
  density   C = 1,  channel-first 160^3, M = 8192 rays x 256 samples = 2 097 152
  k0        C = 12, channels-last 160^3, M =  800 rays x 256 samples =   204 800
Positions are ray-ordered, as the sampler writes them: the chords of scenes.roofline_rays through the box, 256 steps each.
  hip    the kernel alone through the C ABI, on the layout the model stores (channel-first for C = 1, channels-last else)
  torch  aten::grid_sampler_3d_backward(grad_out, volume [1,C,X,Y,Z] contiguous, ind_norm [1,1,1,M,3], bilinear, zeros,
         align_corners=True, output_mask=[False, True]) called directly -- the kernel F.grid_sample's backward runs, without
         the autograd engine around it; it still allocates its result each call.  The forward and the chain rule from
         ind_norm back to world positions are NOT in the timed region (the hip kernel's scale is)
One process, both variants warmed up, alternating within a round; each sample is one device-event pair around `reps`
back-to-back launches (2000 by default: windows of 60-170 ms), so a figure is the time per launch of a full queue: the
kernel, or the host's issue rate where that is slower (`*_host_us`: the host's time per call, measured apart, says which).
Reported: the median over rounds per launch and the spread (max - min of the rounds).  The two results are compared before
timing (max |difference| over max |value|).  Prints one JSON line per case; `--out FILE` also writes them there.

  python tools/xyzgrad_bench.py [--reps 2000] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=2000, help='launches per timed sample')
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--world', type=int, default=160)
ap.add_argument('--out', default=None)
args = ap.parse_args()

import torch  # noqa: E402

from directvoxgo_amd import _lib as L  # noqa: E402
from directvoxgo_amd.scenes import roofline_rays  # noqa: E402

assert torch.cuda.is_available(), 'xyzgrad_bench needs the GPU: a CPU run measures nothing'
HALF = 1.5 * 1.05
CASES = [('density', 1, 8192), ('k0', 12, 800)]


def positions(n_rays, gen, n_samples=256):
    o, d = roofline_rays(n_rays, gen, HALF)
    step = (2 * HALF - 2e-2) / n_samples
    t = (torch.arange(n_samples, dtype=torch.float32) + 0.5) * step
    return (o[:, None, :] + d[:, None, :] * t[None, :, None]).reshape(-1, 3).cuda().contiguous()


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def host_us(fn, reps):
    """the host's time to issue one call (queue drained before and after)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (t1 - t0) / reps * 1e6


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


lines = []
for name, C, n_rays in CASES:
    gen = torch.Generator().manual_seed(777)
    W = args.world
    xyz = positions(n_rays, gen)
    M = xyz.shape[0]
    vol = torch.randn((1, C, W, W, W), generator=gen).cuda()                       # torch's layout
    grid = vol.contiguous(memory_format=torch.channels_last_3d) if C > 1 else vol  # the model's layout
    gout = torch.randn((M, C), generator=gen).cuda()
    mn, mx = torch.full((3,), -HALF).cuda(), torch.full((3,), HALF).cuda()
    out = torch.empty((M, 3), device='cuda')
    _, sC, sX, sY, sZ = grid.stride()
    stream = L.stream_of(xyz)

    def hip():
        L.call('dvgo_grid_sample_bwd_xyz', grid, C, W, W, W, sC, sX, sY, sZ, gout, xyz, mn, mx, M, out, stream)

    ind = (((xyz - mn) / (mx - mn)).flip(-1) * 2 - 1).reshape(1, 1, 1, M, 3).requires_grad_()
    ind = ind.detach()
    g_t = gout.t().reshape(1, C, 1, 1, M).contiguous()

    def torch_bwd():
        return torch.ops.aten.grid_sampler_3d_backward(g_t, vol, ind, 0, 0, True, [False, True])[1]

    hip()
    want = torch_bwd().reshape(M, 3).flip(-1) * (2 / (mx - mn))                    # d ind_norm / d xyz
    diff = float((out - want).abs().max() / want.abs().max())
    for _ in range(3):
        hip(); torch_bwd()
    t = {'hip': [], 'torch': []}
    for _ in range(args.rounds):
        t['hip'].append(timed(hip, args.reps))
        t['torch'].append(timed(torch_bwd, args.reps))
    rec = {'case': name, 'C': C, 'M': M, 'world': W, 'layout': 'channels_last' if C > 1 else 'channel_first',
           'hip_ms': round(median(t['hip']), 4), 'hip_spread_ms': round(max(t['hip']) - min(t['hip']), 4),
           'torch_ms': round(median(t['torch']), 4), 'torch_spread_ms': round(max(t['torch']) - min(t['torch']), 4),
           'hip_host_us': round(host_us(hip, 200), 1), 'torch_host_us': round(host_us(torch_bwd, 200), 1),
           'torch_over_hip': round(median(t['torch']) / median(t['hip']), 3), 'max_rel_diff': diff,
           'reps': args.reps, 'rounds': args.rounds}
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)
    del vol, grid, ind
if args.out:
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
