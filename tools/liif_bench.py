"""Speed of the LIIF plane decoder's kernels (csrc/liif.hip: ops.liif_gather, ops.liif_blend) against what a user runs
without them: the decoder restated op by op in torch (per plane and shift: shift, clamp, two nearest grid_sample, cat; then
the area-weighted sum), with the autograd backward, on the same device and inputs.  The decoder's GEMMs (two InterpMLP
batches, width 128, depth 5, forward + backward, dropout off) are the same in both and timed on their own, so that their
share of a decode is visible.

Positions: the first 2^17 kept samples of the roofline scene (scenes.roofline_scene, 160^3) from the fused march, so
that neighbouring samples are neighbours on a ray.  Cases: planes 160^2 and 200^2, C in {32, 64}, 'sum', cell_decode and
local_ensemble on (configs/nerf/tri_lego.py).  One process, every shape warmed up, the variants alternating within a
round, device-event timing, the median over rounds x reps and the spread (max - min of the per-round medians):
  torch     channel-first planes; fwd = rows + blend of fixed predictions; bwd = autograd of both (fixed gradients)
  hip       ops.liif_gather + ops.liif_blend on channels-last planes (the model's storage); bwd = their backward
  gemm      InterpMLP on inp[0] and on inp[1:3], forward + backward
  scatter_runN   dvgo_liif_scatter alone into zero-filled buffers (the zero fill not timed), merging runs of N samples
Forward bytes: the algorithmic traffic M * (12 D * 4 + 12 * 4 + 12) of the gather plus M * (12 C * 4 + 12 * 4 + C * 4)
of the blend, over the hip forward time.
Prints one JSON line per case and a last line with the verdict; `--out FILE` also writes them there.

  python tools/liif_bench.py [--reps 10] [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=10, help='timed calls per variant and round')
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--samples', type=int, default=1 << 17)
ap.add_argument('--runs', default='1,2,4,8', help='comma list of run lengths for the scatter A/B')
ap.add_argument('--sizes', default='160,200')
ap.add_argument('--channels', default='32,64')
ap.add_argument('--out', default=None)
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from directvoxgo_amd import ops  # noqa: E402
from directvoxgo_amd.fused import fused_march  # noqa: E402
from directvoxgo_amd.liif import InterpMLP  # noqa: E402
from directvoxgo_amd.scenes import roofline_scene  # noqa: E402
from directvoxgo_amd.triplane import TriPlaneVoxGO  # noqa: E402

assert torch.cuda.is_available(), 'liif_bench needs the GPU: a CPU run measures nothing'
KEYS = ('xy', 'yz', 'zx')
TABLE = {'xy': (2, 1, 0, 1), 'yz': (1, 0, 1, 2), 'zx': (0, 2, 2, 0)}      # world axis of u, of v; world_size index of Ta, Tb
SHIFTS = ((-1, -1), (-1, 1), (1, -1), (1, 1))
RUNS = [int(v) for v in args.runs.split(',')]
WS = (160, 160, 160)


def positions():
    sc = roofline_scene(world=160, n_rays=8192, device='cuda')
    m = TriPlaneVoxGO(sc['xyz_min'], sc['xyz_max'], num_voxels=160 ** 3, num_voxels_base=160 ** 3, alpha_init=1e-2,
                      fast_color_thres=1e-4, rgbnet_dim=4, plane_size=(8, 8)).cuda()
    assert tuple(int(v) for v in m.world_size) == WS
    with torch.no_grad():
        m.density.copy_(sc['density']); m.mask_cache.mask.copy_(sc['mask'])
        cfg = m._march_cfg(sc['near'], sc['far'], sc['stepsize'])
        pts = fused_march(m.density, m.density.detach()[:, :0], sc['rays_o'], sc['rays_d'], cfg, positions=True)[3]
    assert pts.shape[0] >= args.samples
    return pts[:args.samples].contiguous(), m.xyz_min.clone(), m.xyz_max.clone()


def torch_rows(planes, xyz, mn, mx):
    """-> inp [3, 4, M, C + 4], area [3, 4, M]: the decoder's gathers, one torch op after the other."""
    n = ((xyz - mn) / (mx - mn)) * 2 - 1
    inps, areas = [], []
    for key in KEYS:
        au, av, ia, ib = TABLE[key]
        u, v, (Ta, Tb) = n[:, au], n[:, av], (WS[ia], WS[ib])
        H, W = planes[key].shape[2:]
        rows_t, cols_t = torch.meshgrid(torch.linspace(-1, 1, Ta, device=xyz.device), torch.linspace(-1, 1, Tb, device=xyz.device),
                                        indexing='ij')
        table = torch.stack([cols_t, rows_t])[None]
        cells = torch.stack([torch.full_like(u, H / Ta), torch.full_like(u, W / Tb)], -1)
        for vx, vy in SHIFTS:
            uc = (u + (vx / Ta + 1e-6)).clamp(-1 + 1e-6, 1 - 1e-6)
            vc = (v + (vy / Tb + 1e-6)).clamp(-1 + 1e-6, 1 - 1e-6)
            grid = torch.stack([vc, uc], -1).reshape(1, 1, -1, 2)
            feat = F.grid_sample(planes[key], grid, mode='nearest', align_corners=False)[0, :, 0, :].T
            q = F.grid_sample(table, grid, mode='nearest', align_corners=False)[0, :, 0, :].T
            rel = torch.stack([(u - q[:, 0]) * H, (v - q[:, 1]) * W], -1)
            inps.append(torch.cat([feat, rel, cells], -1))
            areas.append((rel[:, 0] * rel[:, 1]).abs() + 1e-9)
    M = xyz.shape[0]
    return torch.stack(inps).reshape(3, 4, M, -1), torch.stack(areas).reshape(3, 4, M)


def torch_blend(pred, area):
    wgt = area.flip(1) / area.sum(1, keepdim=True)
    per_plane = (pred * wgt[..., None]).sum(1)
    return per_plane[0] + per_plane[1] + per_plane[2]


def hip_fwd(planes, pred, xyz, mn, mx):
    inp, wgt = ops.liif_gather(planes, xyz, mn, mx, WS, True, True)
    return inp, ops.liif_blend(pred, wgt, 'sum')


def torch_fwd(planes, pred, xyz, mn, mx):
    inp, area = torch_rows(planes, xyz, mn, mx)
    return inp, torch_blend(pred, area)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    return r, (a, b)


def glue(fwd, planes, pred, xyz, mn, mx, gout, ginp, reps):
    ev_f, ev_b = [], []
    for _ in range(reps):
        pred.grad = None
        for p in planes.values():
            p.grad = None
        (inp, out), e = timed(lambda: fwd(planes, pred, xyz, mn, mx))
        ev_f.append(e)
        _, e = timed(lambda: torch.autograd.backward([out, inp], [gout, ginp]))
        ev_b.append(e)
        del inp, out
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev_f], [a.elapsed_time(b) for a, b in ev_b]


def gemm(nets, inp, gpred, reps):
    ev = []
    for _ in range(reps):
        for net in nets.values():
            net.zero_grad(set_to_none=True)
        def run():
            E, M, D = inp.shape[1:]
            pred = torch.cat([nets['xy'](inp[0].reshape(E * M, D)), nets['yz'](inp[1:].reshape(2 * E * M, D))])
            pred.backward(gpred)
        ev.append(timed(run)[1])
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def scatter_only(grads, ginp, xyz, mn, mx, run, reps):
    ev = []
    for _ in range(reps):
        for g in grads.values():
            g.zero_()
        ev.append(timed(lambda: ops.liif_gather_bwd(ginp, grads, xyz, mn, mx, WS, True, True, run=run))[1])
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def summary(rounds):
    meds = [float(np.median(r)) for r in rounds]
    return {'median_ms': round(float(np.median(np.concatenate(rounds))), 4), 'spread_ms': round(max(meds) - min(meds), 4)}


xyz, mn, mx = positions()
M = xyz.shape[0]
lines = [{'positions': M, 'source': 'roofline scene 160^3, first kept samples', 'reps': args.reps, 'rounds': args.rounds}]
print(json.dumps(lines[0]), flush=True)
gen = torch.Generator(device='cuda').manual_seed(0)
verdict = []
for S in [int(v) for v in args.sizes.split(',')]:
    for C in [int(v) for v in args.channels.split(',')]:
        D = C + 4
        base = {k: torch.randn((1, C, S, S), generator=gen, device='cuda') * 0.3 for k in KEYS}
        gout = torch.randn((M, C), generator=gen, device='cuda')
        ginp = torch.randn((3, 4, M, D), generator=gen, device='cuda')
        variants = {
            'torch': (torch_fwd, {k: v.clone().requires_grad_() for k, v in base.items()},
                      torch.randn((3, 4, M, C), generator=gen, device='cuda').requires_grad_()),
            'hip': (hip_fwd, {k: v.clone().contiguous(memory_format=torch.channels_last).requires_grad_() for k, v in base.items()},
                    None),
        }
        variants['hip'] = variants['hip'][:2] + (variants['torch'][2].detach().clone().requires_grad_(),)
        nets = {k: InterpMLP(D, C, 128, 5).cuda().eval() for k in ('xy', 'yz')}
        grads = {k: torch.zeros_like(v, memory_format=torch.channels_last) for k, v in base.items()}
        # same results first, then the warm-up of every variant
        with torch.no_grad():
            (ti, to), (hi, ho) = torch_fwd(base, variants['torch'][2], xyz, mn, mx), hip_fwd(base, variants['torch'][2], xyz, mn, mx)
            rows_differ = int((ti != hi).any(-1).sum())
            out_diff = float((to - ho).abs().max())
            inp_fixed = hi.clone()
            del ti, to, hi, ho
        for fn, pl, pr in variants.values():
            glue(fn, pl, pr, xyz, mn, mx, gout, ginp, 2)
        g_ref, g_hip = variants['torch'][1]['xy'].grad, variants['hip'][1]['xy'].grad
        grad_diff = float((g_ref - g_hip).abs().max() / g_ref.abs().max())
        gpred = torch.randn((3 * 4 * M, C), generator=gen, device='cuda')
        gemm(nets, inp_fixed, gpred, 2)
        for run in RUNS:
            scatter_only(grads, ginp, xyz, mn, mx, run, 2)
        T = {v: {'fwd': [], 'bwd': []} for v in variants}
        TG, TR = [], {run: [] for run in RUNS}
        for _ in range(args.rounds):
            for v, (fn, pl, pr) in variants.items():
                f, b = glue(fn, pl, pr, xyz, mn, mx, gout, ginp, args.reps)
                T[v]['fwd'].append(f); T[v]['bwd'].append(b)
            TG.append(gemm(nets, inp_fixed, gpred, args.reps))
            for run in RUNS:
                TR[run].append(scatter_only(grads, ginp, xyz, mn, mx, run, args.reps))
        row = {'plane': S, 'C': C, 'rows_that_differ_from_torch': rows_differ, 'max_abs_diff_out': out_diff,
               'rel_diff_grad_xy': grad_diff}
        for v in variants:
            row[v] = {'fwd': summary(T[v]['fwd']), 'bwd': summary(T[v]['bwd'])}
        row['gemm_fwd_bwd'] = summary(TG)
        row['scatter_kernel_by_run'] = {str(run): summary(TR[run]) for run in RUNS}
        fwd_bytes = M * (12 * D * 4 + 12 * 4 + 12) + M * (12 * C * 4 + 12 * 4 + C * 4)
        row['fwd_algorithmic_bytes'] = fwd_bytes
        row['hip_fwd_TBps'] = round(fwd_bytes / (row['hip']['fwd']['median_ms'] * 1e-3) / 1e12, 3)
        row['atomic_bytes'] = M * 12 * C * 4
        for d in ('fwd', 'bwd'):
            spread = max(row['hip'][d]['spread_ms'], row['torch'][d]['spread_ms'])
            ok = row['hip'][d]['median_ms'] <= row['torch'][d]['median_ms'] + spread
            verdict.append(ok)
            row[f'hip_{d}_no_slower_than_torch'] = ok
        lines.append(row)
        print(json.dumps(row), flush=True)
        del variants, grads, base, gout, ginp, nets, inp_fixed, gpred
        torch.cuda.empty_cache()
lines.append({'every_case_meets_the_bar': all(verdict), 'cases': len(verdict)})
print(json.dumps(lines[-1]), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        for ln in lines:
            fh.write(json.dumps(ln) + '\n')
