"""Speed of the bilinear plane decoder's kernels (csrc/plane_rows.hip: ops.plane_rows forward and backward) against what a
user runs without them: the decoder's rows restated op by op in torch as the reference builds them (per plane one
bilinear F.grid_sample on the plane, the coordinate table rebuilt with linspace / meshgrid, one bilinear F.grid_sample on
it, the sin / cos encoding, the cat), with the autograd backward into the planes, on the same device and inputs.  The
decoder's GEMMs (two InterpMLP batches, width 128, depth 3, forward + backward, dropout off) are the same in both and timed
on their own, so that their share of a decode is visible.

Shape: configs/nerf/tri_multiscene.py -- C = 64, posbase_pe = 5, cell_decode (D = 88), planes and world_size 160.
Positions: kept samples of the roofline scene (scenes.roofline_scene, 160^3) from the fused march, so that neighbouring
samples are neighbours on a ray: all kept samples of one fine-stage batch (N_rand = 4096 rays), and the first 2^17 of an
8192-ray batch.  One process, every shape warmed up, the variants alternating within a round, device-event timing, the
median over rounds x reps and the spread (max - min of the per-round medians):
  torch     channel-first planes; fwd = the rows; bwd = autograd into the planes (fixed gradient)
  hip       ops.plane_rows on channels-last planes (the model's storage); bwd = its backward (zero fill + scatter)
  gemm      InterpMLP on inp[0] and on inp[1:3], forward + backward
Forward bytes: the algorithmic traffic M * (3 D * 4 + 12) over the time of the hip forward CALL (allocation, autograd
function and launch included): a call-level rate, not the kernel's achieved bandwidth.
Prints one JSON line per case and a last line with the verdict; `--out FILE` also writes them there.

  python tools/interp_bench.py [--reps 10] [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=10, help='timed calls per variant and round')
ap.add_argument('--rounds', type=int, default=3)
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

assert torch.cuda.is_available(), 'interp_bench needs the GPU: a CPU run measures nothing'
KEYS = ('xy', 'yz', 'zx')
AXES = {'xy': (1, 2), 'yz': (0, 1), 'zx': (2, 0)}          # world axis of the rows, of the columns
TABLE = {'xy': (0, 1), 'yz': (1, 2), 'zx': (2, 0)}         # world_size index of Ta, Tb
WS = (160, 160, 160)
C, P, S = 64, 5, 160
D = C + 2 + 4 * P + 2


def positions(n_rays, limit=None):
    sc = roofline_scene(world=160, n_rays=n_rays, device='cuda')
    m = TriPlaneVoxGO(sc['xyz_min'], sc['xyz_max'], num_voxels=160 ** 3, num_voxels_base=160 ** 3, alpha_init=1e-2,
                      fast_color_thres=1e-4, rgbnet_dim=4, plane_size=(8, 8)).cuda()
    assert tuple(int(v) for v in m.world_size) == WS
    with torch.no_grad():
        m.density.copy_(sc['density']); m.mask_cache.mask.copy_(sc['mask'])
        cfg = m._march_cfg(sc['near'], sc['far'], sc['stepsize'])
        pts = fused_march(m.density, m.density.detach()[:, :0], sc['rays_o'], sc['rays_d'], cfg, positions=True)[3]
    if limit is not None:
        assert pts.shape[0] >= limit
        pts = pts[:limit]
    return pts.contiguous(), m.xyz_min.clone(), m.xyz_max.clone()


def torch_rows(planes, xyz, mn, mx):
    """-> inp [3, M, D]: the decoder's rows, one torch op after the other, the table rebuilt per call as make_coord does"""
    n = ((xyz - mn) / (mx - mn)) * 2 - 1
    freq = 2.0 ** torch.arange(P, device=xyz.device, dtype=torch.float32)
    inps = []
    for key in KEYS:
        ah, aw = AXES[key]
        Ta, Tb = WS[TABLE[key][0]], WS[TABLE[key][1]]
        grid = torch.stack([n[:, aw], n[:, ah]], -1).reshape(1, 1, -1, 2)
        feat = F.grid_sample(planes[key], grid, mode='bilinear', align_corners=True)[0, :, 0, :].T
        rows_t, cols_t = torch.meshgrid(torch.linspace(-1, 1, Ta, device=xyz.device), torch.linspace(-1, 1, Tb, device=xyz.device),
                                        indexing='ij')
        table = torch.stack([cols_t, rows_t])[None]
        q = F.grid_sample(table, grid, mode='bilinear', align_corners=True)[0, :, 0, :].T
        emb = (q.unsqueeze(-1) * freq).flatten(-2)
        cell = torch.zeros(xyz.shape[0], 2, device=xyz.device)
        cell[:, 0] = 1.0 / Ta
        cell[:, 1] = 1.0 / Tb
        inps.append(torch.cat([feat, q, emb.sin(), emb.cos(), cell], -1))
    return torch.stack(inps)


def hip_rows(planes, xyz, mn, mx):
    return ops.plane_rows(planes, xyz, mn, mx, WS, P, True)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    return r, (a, b)


def glue(fwd, planes, xyz, mn, mx, ginp, reps):
    ev_f, ev_b = [], []
    for _ in range(reps):
        for p in planes.values():
            p.grad = None
        inp, e = timed(lambda: fwd(planes, xyz, mn, mx))
        ev_f.append(e)
        _, e = timed(lambda: inp.backward(ginp))
        ev_b.append(e)
        del inp
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev_f], [a.elapsed_time(b) for a, b in ev_b]


def gemm(nets, inp, gpred, reps):
    ev = []
    for _ in range(reps):
        for net in nets.values():
            net.zero_grad(set_to_none=True)

        def run():
            M = inp.shape[1]
            pred = torch.cat([nets['xy'](inp[0]), nets['yz'](inp[1:].reshape(2 * M, D))])
            pred.backward(gpred)
        ev.append(timed(run)[1])
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def summary(rounds):
    meds = [float(np.median(r)) for r in rounds]
    return {'median_ms': round(float(np.median(np.concatenate(rounds))), 4), 'spread_ms': round(max(meds) - min(meds), 4)}


lines = [{'C': C, 'posbase_pe': P, 'D': D, 'plane': S, 'world_size': WS, 'reps': args.reps, 'rounds': args.rounds}]
print(json.dumps(lines[0]), flush=True)
gen = torch.Generator(device='cuda').manual_seed(0)
verdict = []
for label, n_rays, limit in (('fine-stage batch, 4096 rays, all kept samples', 4096, None), ('8192 rays, first 2^17 kept samples', 8192, 1 << 17)):
    xyz, mn, mx = positions(n_rays, limit)
    M = xyz.shape[0]
    base = {k: torch.randn((1, C, S, S), generator=gen, device='cuda') * 0.3 for k in KEYS}
    ginp = torch.randn((3, M, D), generator=gen, device='cuda')
    variants = {
        'torch': (torch_rows, {k: v.clone().requires_grad_() for k, v in base.items()}),
        'hip': (hip_rows, {k: v.clone().contiguous(memory_format=torch.channels_last).requires_grad_() for k, v in base.items()}),
    }
    nets = {k: InterpMLP(D, C, 128, 3).cuda().eval() for k in ('xy', 'yz')}
    with torch.no_grad():      # same results first, then the warm-up of every variant
        ti, hi = torch_rows(base, xyz, mn, mx), hip_rows(base, xyz, mn, mx)
        max_diff = float((ti - hi).abs().max())
        inp_fixed = hi.clone()
        del ti, hi
    for fn, pl in variants.values():
        glue(fn, pl, xyz, mn, mx, ginp, 2)
    g_ref, g_hip = variants['torch'][1]['xy'].grad, variants['hip'][1]['xy'].grad
    grad_diff = float((g_ref - g_hip).abs().max() / g_ref.abs().max())
    gpred = torch.randn((3 * M, C), generator=gen, device='cuda')
    gemm(nets, inp_fixed, gpred, 2)
    T = {v: {'fwd': [], 'bwd': []} for v in variants}
    TG = []
    for _ in range(args.rounds):
        for v, (fn, pl) in variants.items():
            f, b = glue(fn, pl, xyz, mn, mx, ginp, args.reps)
            T[v]['fwd'].append(f); T[v]['bwd'].append(b)
        TG.append(gemm(nets, inp_fixed, gpred, args.reps))
    row = {'positions': M, 'source': label, 'max_abs_diff_rows': max_diff, 'rel_diff_grad_xy': grad_diff}
    for v in variants:
        row[v] = {'fwd': summary(T[v]['fwd']), 'bwd': summary(T[v]['bwd'])}
    row['gemm_fwd_bwd'] = summary(TG)
    fwd_bytes = M * (3 * D * 4 + 12)
    row['fwd_algorithmic_bytes'] = fwd_bytes
    row['hip_fwd_TBps'] = round(fwd_bytes / (row['hip']['fwd']['median_ms'] * 1e-3) / 1e12, 3)
    row['atomic_bytes'] = M * 12 * C * 4
    for d in ('fwd', 'bwd'):
        spread = max(row['hip'][d]['spread_ms'], row['torch'][d]['spread_ms'])
        ok = row['hip'][d]['median_ms'] <= row['torch'][d]['median_ms'] + spread
        verdict.append(ok)
        row[f'hip_{d}_no_slower_than_torch'] = ok
        row[f'torch_over_hip_{d}'] = round(row['torch'][d]['median_ms'] / row['hip'][d]['median_ms'], 2)
    lines.append(row)
    print(json.dumps(row), flush=True)
    del variants, base, ginp, nets, inp_fixed, gpred
    torch.cuda.empty_cache()
lines.append({'every_case_meets_the_bar': all(verdict), 'cases': len(verdict)})
print(json.dumps(lines[-1]), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        for ln in lines:
            fh.write(json.dumps(ln) + '\n')
