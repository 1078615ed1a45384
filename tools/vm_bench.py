"""Speed of the vector-matrix sampler (csrc/vm.hip, ops.vm_sample) against what a user runs without it: six F.grid_sample
calls (three planes, three lines), the product and the cat, with the autograd backward, on the same device and inputs.

Positions: the kept samples of the roofline scene (scenes.roofline_scene: 8192 rays x 256 samples = 2 097 152) and of a
lego-like batch (scenes.synthetic_scene at 160^3, 8192 rays), both from the fused march.  Shapes: R in {16, 48}, planes
160^2, lines 160.  The protocol of tools/triplane_bench.py: one process, every shape warmed up, the variants alternating
within a round, device-event timing, the median over rounds x reps and the spread (max - min of the per-round medians)
reported per variant:
  torch      channel-first planes and lines (torch's layout), grid_sample x 6, product, cat; backward by autograd
  hip        ops.vm_sample on channels-last planes and lines (VMTriPlaneVoxGO's own storage); the backward is the kernel in
             mode 0 / run 0 behind six zero fills
  bwd_mK_rN  the backward kernel alone (ops.vm_bwd into zero-filled channels-last buffers, the zero fill not timed), mode K
             in {1, 2} with a lane merging runs of N consecutive samples; 'illegal' where mode 2's table exceeds 64 KB
Atomic bytes: the unmerged count, M * 3R * 6 * 4, over the kernel's time, beside the chip-wide float-atomic rate of about
1.3 TB/s.  `--train` also times one TrainStep of VMTriPlaneVoxGO(n_comp=16, rgbnet_dim=12) beside TriPlaneVoxGO(rgbnet_dim=16,
'concat') on the lego-like scene, for orientation.  Prints one JSON line per case and a last line with the verdict;
`--out FILE` also writes them there.

  python tools/vm_bench.py [--reps 10] [--rounds 3] [--train] [--out FILE]
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
ap.add_argument('--modes', default='1,2', help='comma list of backward modes for the A/B')
ap.add_argument('--size', type=int, default=160, help='plane side and line length')
ap.add_argument('--comps', default='16,48')
ap.add_argument('--scenes', default='roofline,lego')
ap.add_argument('--train', action='store_true', help='also time one TrainStep of the VM model beside the tri-plane model')
ap.add_argument('--out', default=None)
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from directvoxgo_amd import ops  # noqa: E402
from directvoxgo_amd.fused import fused_march  # noqa: E402
from directvoxgo_amd.scenes import roofline_scene, synthetic_scene  # noqa: E402
from directvoxgo_amd.triplane import TRI_FINE_TRAIN, TriPlaneVoxGO  # noqa: E402

assert torch.cuda.is_available(), 'vm_bench needs the GPU: a CPU run measures nothing'
KEYS = ('xy', 'yz', 'zx')
PAIRS = {'xy': [0, 1], 'yz': [1, 2], 'zx': [2, 0]}          # of the flipped triple (n_z, n_y, n_x): (columns, rows)
LINE_OF = {'xy': 2, 'yz': 0, 'zx': 1}                       # index into the flipped triple of the line's world axis (x, z, y)
RUNS = [int(v) for v in args.runs.split(',')]
MODES = [int(v) for v in args.modes.split(',')]
ATOMIC_RATE = 1.3e12


def scene_of(name):
    if name == 'roofline':
        return roofline_scene(world=160, n_rays=args.rays, device='cuda')
    return synthetic_scene(world=160, n_rays=args.rays, device='cuda')


def positions(sc):
    m = TriPlaneVoxGO(sc['xyz_min'], sc['xyz_max'], num_voxels=160 ** 3, num_voxels_base=160 ** 3, alpha_init=1e-2,
                      fast_color_thres=1e-4, rgbnet_dim=4, plane_size=(8, 8)).cuda()
    with torch.no_grad():
        m.density.copy_(sc['density']); m.mask_cache.mask.copy_(sc['mask'])
        cfg = m._march_cfg(sc['near'], sc['far'], sc['stepsize'])
        pts = fused_march(m.density, m.density.detach()[:, :0], sc['rays_o'], sc['rays_d'], cfg, positions=True)[3]
    return pts.contiguous(), m.xyz_min.clone(), m.xyz_max.clone()


def torch_sample(planes, lines, xyz, mn, mx):
    x = xyz.reshape(1, 1, -1, 3)
    ind = ((x - mn) / (mx - mn)).flip((-1,)) * 2 - 1
    out = []
    for k in KEYS:
        p = F.grid_sample(planes[k], ind[..., PAIRS[k]], mode='bilinear', align_corners=True)[0, :, 0, :].T
        along = ind[..., [LINE_OF[k]]]
        ln = F.grid_sample(lines[k], torch.cat([torch.zeros_like(along), along], -1), mode='bilinear', align_corners=True)[0, :, 0, :].T
        out.append(p * ln)
    return torch.cat(out, -1)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    return r, (a, b)


def fwd_bwd(sample, planes, lines, xyz, mn, mx, gout, reps):
    ev_f, ev_b = [], []
    for _ in range(reps):
        for p in list(planes.values()) + list(lines.values()):
            p.grad = None
        out, e = timed(lambda: sample(planes, lines, xyz, mn, mx))
        ev_f.append(e)
        _, e = timed(lambda: out.backward(gout))
        ev_b.append(e)
        del out
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev_f], [a.elapsed_time(b) for a, b in ev_b]


def bwd_only(planes, lines, gp, gl, xyz, mn, mx, gout, run, mode, reps):
    ev = []
    for _ in range(reps):
        for g in list(gp.values()) + list(gl.values()):
            g.zero_()
        ev.append(timed(lambda: ops.vm_bwd(gout, planes, lines, gp, gl, xyz, mn, mx, run=run, mode=mode))[1])
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def summary(rounds):
    """rounds: per round, the list of times -> median over everything, spread of the per-round medians"""
    meds = [float(np.median(r)) for r in rounds]
    return {'median_ms': round(float(np.median(np.concatenate(rounds))), 4), 'spread_ms': round(max(meds) - min(meds), 4)}


def train_step_times(sc):
    """One TrainStep (forward, backward, optimizer) of each model on the scene's rays: median of 10 after 3 warm-ups."""
    from directvoxgo_amd.train import TrainStep
    from directvoxgo_amd.vm import VM_FINE_TRAIN, VMTriPlaneVoxGO
    common = dict(num_voxels=160 ** 3, num_voxels_base=160 ** 3, alpha_init=1e-2, fast_color_thres=1e-4)
    rk = dict(near=sc['near'], far=sc['far'], bg=1, stepsize=sc['stepsize'])
    out = {}
    for name, make, cfg in (('vm_n16_c12', lambda: VMTriPlaneVoxGO(sc['xyz_min'], sc['xyz_max'], n_comp=16, rgbnet_dim=12, **common), VM_FINE_TRAIN),
                            ('triplane_c16_concat', lambda: TriPlaneVoxGO(sc['xyz_min'], sc['xyz_max'], rgbnet_dim=16, **common), TRI_FINE_TRAIN)):
        torch.manual_seed(0)
        m = make().cuda()
        with torch.no_grad():
            m.density.copy_(sc['density']); m.mask_cache.mask.copy_(sc['mask'])
        step = TrainStep(m, dict(cfg), rk)
        a = (sc['rays_o'], sc['rays_d'], sc['viewdirs'], sc['target'])
        for s in range(3):
            step(*a, global_step=s + 1)
        ev = [timed(lambda: step(*a, global_step=4 + s))[1] for s in range(10)]
        torch.cuda.synchronize()
        out[name] = {'median_ms': round(float(np.median([x.elapsed_time(y) for x, y in ev])), 3)}
        del m, step
        torch.cuda.empty_cache()
    return out


lines_out = [{'reps': args.reps, 'rounds': args.rounds, 'plane': args.size, 'line': args.size}]
print(json.dumps(lines_out[0]), flush=True)
gen = torch.Generator(device='cuda').manual_seed(0)
verdict = []
S = args.size
for scene in args.scenes.split(','):
    sc = scene_of(scene)
    xyz, mn, mx = positions(sc)
    M = xyz.shape[0]
    for R in [int(v) for v in args.comps.split(',')]:
        base_p = {k: torch.randn((1, R, S, S), generator=gen, device='cuda') * 0.3 for k in KEYS}
        base_l = {k: torch.randn((1, R, S, 1), generator=gen, device='cuda') * 0.3 for k in KEYS}
        gout = torch.randn((M, 3 * R), generator=gen, device='cuda')
        cl = lambda d: {k: v.clone().contiguous(memory_format=torch.channels_last) for k, v in d.items()}          # noqa: E731
        rg = lambda d: {k: v.requires_grad_() for k, v in d.items()}                                               # noqa: E731
        variants = {'torch': (torch_sample, rg({k: v.clone() for k, v in base_p.items()}), rg({k: v.clone() for k, v in base_l.items()})),
                    'hip': (ops.vm_sample, rg(cl(base_p)), rg(cl(base_l)))}
        vp, vl = cl(base_p), cl(base_l)
        gp, gl = {k: torch.zeros_like(v) for k, v in vp.items()}, {k: torch.zeros_like(v) for k, v in vl.items()}
        legal = {mode: mode != 2 or 3 * S * R * 4 <= 64 * 1024 for mode in MODES}
        ab = [(mode, run) for mode in MODES if legal[mode] for run in RUNS]
        # same results first, then the warm-up of every variant
        with torch.no_grad():
            ref = torch_sample(base_p, base_l, xyz, mn, mx)
            got = ops.vm_sample(base_p, base_l, xyz, mn, mx)
            max_diff = float((ref - got).abs().max())
            del ref, got
        for fn, pl, ln in variants.values():
            fwd_bwd(fn, pl, ln, xyz, mn, mx, gout, 2)
        gdiff = {}
        for what, i in (('plane_xy', 1), ('line_xy', 2)):
            g_ref, g_hip = variants['torch'][i]['xy'].grad, variants['hip'][i]['xy'].grad
            gdiff[what] = float((g_ref - g_hip).abs().max() / g_ref.abs().max())
        for mode, run in ab:
            bwd_only(vp, vl, gp, gl, xyz, mn, mx, gout, run, mode, 2)
        if legal.get(2) and 1 in MODES:                   # the two modes against each other
            for g in list(gp.values()) + list(gl.values()):
                g.zero_()
            ops.vm_bwd(gout, vp, vl, gp, gl, xyz, mn, mx, run=4, mode=1)
            one = [g.clone() for g in gl.values()]
            for g in list(gp.values()) + list(gl.values()):
                g.zero_()
            ops.vm_bwd(gout, vp, vl, gp, gl, xyz, mn, mx, run=4, mode=2)
            gdiff['line_mode2_vs_mode1'] = max(float((a - b).abs().max() / a.abs().max()) for a, b in zip(one, gl.values()))
            del one
        T = {v: {'fwd': [], 'bwd': []} for v in variants}
        TR = {k: [] for k in ab}
        for _ in range(args.rounds):
            for v, (fn, pl, ln) in variants.items():
                f, b = fwd_bwd(fn, pl, ln, xyz, mn, mx, gout, args.reps)
                T[v]['fwd'].append(f); T[v]['bwd'].append(b)
            for mode, run in ab:
                TR[(mode, run)].append(bwd_only(vp, vl, gp, gl, xyz, mn, mx, gout, run, mode, args.reps))
        row = {'scene': scene, 'positions': M, 'R': R, 'max_abs_diff_fwd': max_diff, 'rel_diff_grad': gdiff}
        for v in variants:
            row[v] = {'fwd': summary(T[v]['fwd']), 'bwd': summary(T[v]['bwd'])}
        atomic_bytes = M * 3 * R * 6 * 4
        row['atomic_bytes_unmerged'] = atomic_bytes
        row['bwd_kernel'] = {}
        for mode in MODES:
            for run in RUNS:
                key = f'm{mode}_r{run}'
                if not legal[mode]:
                    row['bwd_kernel'][key] = 'illegal: the table exceeds 64 KB'
                    continue
                s = summary(TR[(mode, run)])
                s['unmerged_atomic_TBps'] = round(atomic_bytes / (s['median_ms'] * 1e-3) / 1e12, 3)
                row['bwd_kernel'][key] = s
        fwd_bytes = M * (4 * 3 * R + 12)
        row['hip_fwd_TBps'] = round(fwd_bytes / (row['hip']['fwd']['median_ms'] * 1e-3) / 1e12, 3)
        row['atomic_floor_ms_at_1.3TBps'] = round(atomic_bytes / ATOMIC_RATE * 1e3, 3)
        for d in ('fwd', 'bwd'):
            spread = max(row['hip'][d]['spread_ms'], row['torch'][d]['spread_ms'])
            ok = row['hip'][d]['median_ms'] <= row['torch'][d]['median_ms'] + spread
            verdict.append(ok)
            row[f'hip_{d}_no_slower_than_torch'] = ok
        lines_out.append(row)
        print(json.dumps(row), flush=True)
        del variants, vp, vl, gp, gl, base_p, base_l, gout
        torch.cuda.empty_cache()
    if args.train and scene == 'lego':
        row = {'scene': scene, 'train_step': train_step_times(sc)}
        lines_out.append(row)
        print(json.dumps(row), flush=True)
    del sc, xyz
    torch.cuda.empty_cache()
lines_out.append({'every_case_meets_the_bar': all(verdict), 'cases': len(verdict)})
print(json.dumps(lines_out[-1]), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        for ln in lines_out:
            fh.write(json.dumps(ln) + '\n')
