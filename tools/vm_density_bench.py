"""Speed of the vector-matrix density (csrc/vm_density.hip, ops.vm_density) against the form the library could already
express: `ops.vm_sample(planes, lines, xyz, ...).sum(-1)` with its autograd backward, on the same device and inputs.

Positions: tools/vm_bench.py's two sets, the kept samples of the roofline scene (8192 rays x 256 samples = 2 097 152) and
of a lego-like batch (scenes.synthetic_scene at 160^3, 8192 rays).  Shapes: R = 16, planes 160^2, lines 160, channels-last.
Incoming gradients: a dense random grad_out [M], and one with the lego-like fraction of exact zeros, placed at random: the
share of the samples behind the occupancy lookup of the lego-like batch that the alpha and weight filters drop, which is what
autograd hands the op in a render.  The protocol of tools/vm_bench.py: one process, everything warmed up, the variants
alternating within a round, device-event timing, the median over rounds x reps and the spread (max - min of the per-round
medians) per variant:
  sum        ops.vm_sample(...).sum(-1); the backward is autograd's: the broadcast of grad_out to [M, 3R], then dvgo_vm_bwd
  density    ops.vm_density; the backward is dvgo_vm_density_bwd in mode 0 / run 0 behind six zero fills
  bwd_mK_rN  the density's backward kernel alone (zero fill not timed), mode K with runs of N samples per lane
The bar: `density` is no slower than `sum`, forward and backward, in every case, the larger of the two spreads being the
only margin.  `--train` also times one TrainStep of TensoRFVoxGO beside VMTriPlaneVoxGO at 160^3 on the lego-like scene, for
orientation.  Prints one JSON line per case and a last line with the verdict; `--out FILE` also writes them there.

  python tools/vm_density_bench.py [--reps 10] [--rounds 3] [--train] [--out FILE]
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
ap.add_argument('--runs', default='1,4,8', help='comma list of run lengths for the backward A/B')
ap.add_argument('--modes', default='1,2', help='comma list of backward modes for the A/B')
ap.add_argument('--size', type=int, default=160, help='plane side and line length')
ap.add_argument('--comp', type=int, default=16)
ap.add_argument('--scenes', default='roofline,lego')
ap.add_argument('--train', action='store_true', help='also time one TrainStep of TensoRFVoxGO beside VMTriPlaneVoxGO')
ap.add_argument('--out', default=None)
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from directvoxgo_amd import ops  # noqa: E402
from directvoxgo_amd.fused import fused_march  # noqa: E402
from directvoxgo_amd.scenes import roofline_scene, synthetic_scene  # noqa: E402
from directvoxgo_amd.triplane import TriPlaneVoxGO  # noqa: E402

assert torch.cuda.is_available(), 'vm_density_bench needs the GPU: a CPU run measures nothing'
KEYS = ('xy', 'yz', 'zx')
RUNS = [int(v) for v in args.runs.split(',')]
MODES = [int(v) for v in args.modes.split(',')]


def scene_of(name):
    if name == 'roofline':
        return roofline_scene(world=160, n_rays=args.rays, device='cuda')
    return synthetic_scene(world=160, n_rays=args.rays, device='cuda')


def positions(sc):
    """-> the kept samples' positions, the box, and (samples behind the occupancy lookup, samples kept)"""
    m = TriPlaneVoxGO(sc['xyz_min'], sc['xyz_max'], num_voxels=160 ** 3, num_voxels_base=160 ** 3, alpha_init=1e-2,
                      fast_color_thres=1e-4, rgbnet_dim=4, plane_size=(8, 8)).cuda()
    with torch.no_grad():
        m.density.copy_(sc['density']); m.mask_cache.mask.copy_(sc['mask'])
        cfg = m._march_cfg(sc['near'], sc['far'], sc['stepsize'])
        pts = fused_march(m.density, m.density.detach()[:, :0], sc['rays_o'], sc['rays_d'], cfg, positions=True)[3]
        every = m.sample_ray(rays_o=sc['rays_o'], rays_d=sc['rays_d'], near=sc['near'], far=sc['far'], stepsize=sc['stepsize'])[0]
        behind = int(m.mask_cache(every).sum())
    return pts.contiguous(), m.xyz_min.clone(), m.xyz_max.clone(), (behind, pts.shape[0])


def sum_of_sampler(planes, lines, xyz, mn, mx):
    return ops.vm_sample(planes, lines, xyz, mn, mx).sum(-1)


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
        ev.append(timed(lambda: ops.vm_density_bwd(gout, planes, lines, gp, gl, xyz, mn, mx, run=run, mode=mode))[1])
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def summary(rounds):
    """rounds: per round, the list of times -> median over everything, spread of the per-round medians"""
    meds = [float(np.median(r)) for r in rounds]
    return {'median_ms': round(float(np.median(np.concatenate(rounds))), 4), 'spread_ms': round(max(meds) - min(meds), 4)}


def train_step_times(sc):
    """One TrainStep (forward, backward, optimizer) of each model on the scene's rays: median of 10 after 3 warm-ups.  The
    VM model marches the scene's dense density; TensoRFVoxGO has none to copy it into and runs on its initial density
    planes behind the scene's occupancy mask, where every sample behind the mask survives the alpha filter."""
    from directvoxgo_amd.tensorf import TENSORF_FINE_TRAIN, TensoRFVoxGO
    from directvoxgo_amd.train import TrainStep
    from directvoxgo_amd.vm import VM_FINE_TRAIN, VMTriPlaneVoxGO
    common = dict(num_voxels=160 ** 3, num_voxels_base=160 ** 3, alpha_init=1e-2, fast_color_thres=1e-4, n_comp=16, rgbnet_dim=12)
    rk = dict(near=sc['near'], far=sc['far'], bg=1, stepsize=sc['stepsize'])
    out = {}
    for name, make, cfg in (('vm_n16_c12', lambda: VMTriPlaneVoxGO(sc['xyz_min'], sc['xyz_max'], **common), VM_FINE_TRAIN),
                            ('tensorf_n16_c12_d16', lambda: TensoRFVoxGO(sc['xyz_min'], sc['xyz_max'], density_n_comp=16, **common),
                             TENSORF_FINE_TRAIN)):
        torch.manual_seed(0)
        m = make().cuda()
        with torch.no_grad():
            if m.density is not None:
                m.density.copy_(sc['density'])
            m.mask_cache.mask.copy_(sc['mask'])
        step = TrainStep(m, dict(cfg), rk)
        a = (sc['rays_o'], sc['rays_d'], sc['viewdirs'], sc['target'])
        for s in range(3):
            step(*a, global_step=s + 1)
        ev = [timed(lambda: step(*a, global_step=4 + s))[1] for s in range(10)]
        torch.cuda.synchronize()
        with torch.no_grad():
            n = int(m(*a[:3], **rk)['ray_id'].shape[0])
        out[name] = {'median_ms': round(float(np.median([x.elapsed_time(y) for x, y in ev])), 3), 'samples_to_colour_head': n}
        del m, step
        torch.cuda.empty_cache()
    return out


lines_out = [{'reps': args.reps, 'rounds': args.rounds, 'plane': args.size, 'line': args.size, 'R': args.comp}]
print(json.dumps(lines_out[0]), flush=True)
gen = torch.Generator(device='cuda').manual_seed(0)
verdict = []
S, R = args.size, args.comp
scenes = {name: scene_of(name) for name in args.scenes.split(',')}
sets = {name: positions(sc) for name, sc in scenes.items()}
# the lego-like fraction of exact zeros: of the samples behind the occupancy lookup, those the filters drop
behind, kept = sets['lego'][3] if 'lego' in sets else next(iter(sets.values()))[3]
zero_fraction = 1.0 - kept / max(behind, 1)
lines_out.append({'lego_like_samples_behind_occupancy': behind, 'kept': kept, 'zero_fraction': round(zero_fraction, 4)})
print(json.dumps(lines_out[-1]), flush=True)
for scene, (xyz, mn, mx, _) in sets.items():
    M = xyz.shape[0]
    base_p = {k: torch.randn((1, R, S, S), generator=gen, device='cuda') * 0.3 for k in KEYS}
    base_l = {k: torch.randn((1, R, S, 1), generator=gen, device='cuda') * 0.3 for k in KEYS}
    cl = lambda d: {k: v.clone().contiguous(memory_format=torch.channels_last) for k, v in d.items()}          # noqa: E731
    rg = lambda d: {k: v.requires_grad_() for k, v in d.items()}                                               # noqa: E731
    dense = torch.randn((M,), generator=gen, device='cuda')
    sparse = dense * (torch.rand((M,), generator=gen, device='cuda') >= zero_fraction)
    for grad_name, gout in (('dense', dense), ('sparse', sparse)):
        variants = {'sum': (sum_of_sampler, rg(cl(base_p)), rg(cl(base_l))),
                    'density': (ops.vm_density, rg(cl(base_p)), rg(cl(base_l)))}
        vp, vl = cl(base_p), cl(base_l)
        gp, gl = {k: torch.zeros_like(v) for k, v in vp.items()}, {k: torch.zeros_like(v) for k, v in vl.items()}
        legal = {mode: mode != 2 or 3 * S * R * 4 <= 64 * 1024 for mode in MODES}
        ab = [(mode, run) for mode in MODES if legal[mode] for run in RUNS]
        with torch.no_grad():                              # same results first, then the warm-up of every variant
            ref = sum_of_sampler(vp, vl, xyz, mn, mx)
            got = ops.vm_density(vp, vl, xyz, mn, mx)
            max_diff = float((ref - got).abs().max())
            del ref, got
        for fn, pl, ln in variants.values():
            fwd_bwd(fn, pl, ln, xyz, mn, mx, gout, 2)
        gdiff = {}
        for what, i in (('plane_xy', 1), ('line_xy', 2)):
            g_ref, g_new = variants['sum'][i]['xy'].grad, variants['density'][i]['xy'].grad
            gdiff[what] = float((g_ref - g_new).abs().max() / g_ref.abs().max())
        for mode, run in ab:
            bwd_only(vp, vl, gp, gl, xyz, mn, mx, gout, run, mode, 2)
        T = {v: {'fwd': [], 'bwd': []} for v in variants}
        TR = {k: [] for k in ab}
        for _ in range(args.rounds):
            for v, (fn, pl, ln) in variants.items():
                f, b = fwd_bwd(fn, pl, ln, xyz, mn, mx, gout, args.reps)
                T[v]['fwd'].append(f); T[v]['bwd'].append(b)
            for mode, run in ab:
                TR[(mode, run)].append(bwd_only(vp, vl, gp, gl, xyz, mn, mx, gout, run, mode, args.reps))
        row = {'scene': scene, 'positions': M, 'R': R, 'grad_out': grad_name, 'zeros': int((gout == 0).sum()),
               'max_abs_diff_fwd': max_diff, 'rel_diff_grad': gdiff}
        for v in variants:
            row[v] = {'fwd': summary(T[v]['fwd']), 'bwd': summary(T[v]['bwd'])}
        row['bwd_kernel'] = {}
        for mode in MODES:
            for run in RUNS:
                key = f'm{mode}_r{run}'
                row['bwd_kernel'][key] = summary(TR[(mode, run)]) if legal[mode] else 'illegal: the table exceeds 64 KB'
        # the forward's algorithmic bytes: what it must move (positions in, one float out, every table once) and what its
        # gathers ask the caches for (3R components x (4 corners + 2 nodes) x 4 bytes per sample)
        tables = 4 * R * (3 * S * S + 3 * S)
        t = row['density']['fwd']['median_ms'] * 1e-3
        row['fwd_bytes_compulsory'] = M * 16 + tables
        row['fwd_bytes_gathered'] = M * 3 * R * 6 * 4
        row['fwd_compulsory_TBps'] = round(row['fwd_bytes_compulsory'] / t / 1e12, 4)
        row['fwd_gathered_TBps'] = round(row['fwd_bytes_gathered'] / t / 1e12, 3)
        row['sum_intermediate_bytes'] = M * 3 * R * 4
        for d in ('fwd', 'bwd'):
            spread = max(row['density'][d]['spread_ms'], row['sum'][d]['spread_ms'])
            ok = row['density'][d]['median_ms'] <= row['sum'][d]['median_ms'] + spread
            verdict.append(ok)
            row[f'density_{d}_no_slower_than_sum'] = ok
        lines_out.append(row)
        print(json.dumps(row), flush=True)
        del variants, vp, vl, gp, gl
        torch.cuda.empty_cache()
    del base_p, base_l, dense, sparse
    torch.cuda.empty_cache()
if args.train and 'lego' in scenes:
    row = {'scene': 'lego', 'train_step': train_step_times(scenes['lego'])}
    lines_out.append(row)
    print(json.dumps(row), flush=True)
lines_out.append({'every_case_meets_the_bar': all(verdict), 'cases': len(verdict)})
print(json.dumps(lines_out[-1]), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        for ln in lines_out:
            fh.write(json.dumps(ln) + '\n')
