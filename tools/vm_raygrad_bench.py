"""Cost of the vector-matrix samplers' position gradient (csrc/vm_xyz.hip: dvgo_vm_bwd_xyz, dvgo_vm_density_bwd_xyz) beside the
forward kernels that gather the same texels (dvgo_vm_fwd, dvgo_vm_density_fwd), and beside the same derivative in torch ops --
six F.grid_sample, products, autograd (tests/vm_oracle.torch_restatement): what a user would write without the kernel.

Positions come from a real march, in ray order: the 8192 x 256 = 2 097 152 samples of scenes.roofline_scene at 160^3.  Planes
160^2, lines 160, R = 16, channels-last (the VEC = 4 path), values N(0, 0.5).  One lane mapping was built (one lane per sample:
csrc/vm_xyz.hip says why), so there is no A/B of mappings.  One process, every variant warmed up, the variants alternating
within a round, device events around each call, the median over rounds x reps and the spread (max - min of the per-round
medians) per variant:
  fwd / density_fwd                 ops.vm_fwd / ops.vm_density_fwd
  bwd_xyz / density_bwd_xyz         ops.vm_bwd_xyz / ops.vm_density_bwd_xyz (the output allocation included)
  torch_ops / density_torch_ops     forward of the restatement plus torch.autograd.grad with respect to the positions
The kernels' results are compared with the restatement's first (largest difference over the largest gradient; float32
F.grid_sample may take the neighbouring cell on a lattice line, so this is a report, not a bound).
`--pose`: one pose.refine_poses iteration (without train_model) of a VMTriPlaneVoxGO(raygrad=True) on the synthetic scene's
density and of a TensoRFVoxGO(raygrad=True) on a density of separable bumps, both 160^3, R = 16, at --rays random pixels of 24
views: CameraRefiner.rays -> model -> train.render_loss -> backward into delta -> Adam on delta.
Prints one JSON line per case; `--out FILE` also writes them there.

  python tools/vm_raygrad_bench.py [--reps 10] [--rounds 3] [--rays 8192] [--pose] [--out FILE]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=10, help='timed calls per variant and round')
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--rays', type=int, default=8192)
ap.add_argument('--pose', action='store_true', help='also time one refine_poses iteration')
ap.add_argument('--out', default=None)
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

import vm_oracle as VO  # noqa: E402
from directvoxgo_amd import ops  # noqa: E402
from directvoxgo_amd.fused import fused_march  # noqa: E402
from directvoxgo_amd.ops import PLANE_KEYS  # noqa: E402
from directvoxgo_amd.scenes import pose_spherical, roofline_scene, synthetic_scene  # noqa: E402
from directvoxgo_amd.tensorf import TENSORF_FINE_TRAIN, TensoRFVoxGO  # noqa: E402
from directvoxgo_amd.vm import VMTriPlaneVoxGO  # noqa: E402

assert torch.cuda.is_available(), 'vm_raygrad_bench needs the GPU: a CPU run measures nothing'
WORLD, R, SIDE = 160, 16, 160
BASE = dict(num_voxels=WORLD ** 3, num_voxels_base=WORLD ** 3, alpha_init=1e-2, fast_color_thres=1e-4)


def positions(sc):
    """The kept samples of the scene's rays, from the fused march, in ray order."""
    m = VMTriPlaneVoxGO(sc['xyz_min'], sc['xyz_max'], n_comp=1, plane_size=(2, 2), line_size=2, **BASE).cuda()
    with torch.no_grad():
        m.density.copy_(sc['density']); m.mask_cache.mask.copy_(sc['mask'])
        cfg = m._march_cfg(sc['near'], sc['far'], sc['stepsize'])
        pts = fused_march(m.density, m.density.detach()[:, :0], sc['rays_o'], sc['rays_d'], cfg, positions=True)[3]
    return pts.contiguous(), m.xyz_min.clone(), m.xyz_max.clone()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def series(fn, reps):
    ev = [timed(fn) for _ in range(reps)]
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
sc = roofline_scene(world=WORLD, n_rays=args.rays, device='cuda')
xyz, mn, mx = positions(sc)
M = xyz.shape[0]
cl = torch.channels_last
planes = {k: (torch.randn((1, R, SIDE, SIDE), generator=gen, device='cuda') * 0.5).contiguous(memory_format=cl) for k in PLANE_KEYS}
vlines = {k: (torch.randn((1, R, SIDE, 1), generator=gen, device='cuda') * 0.5).contiguous(memory_format=cl) for k in PLANE_KEYS}
g_feat = torch.randn((M, 3 * R), generator=gen, device='cuda')
g_dens = torch.randn((M,), generator=gen, device='cuda')


def torch_ops():
    x = xyz.clone().requires_grad_()
    return torch.autograd.grad(VO.torch_restatement(planes, vlines, x, mn, mx), x, g_feat)[0]


def density_torch_ops():
    x = xyz.clone().requires_grad_()
    return torch.autograd.grad(VO.torch_restatement(planes, vlines, x, mn, mx).sum(-1), x, g_dens)[0]


variants = {'fwd': lambda: ops.vm_fwd(planes, vlines, xyz, mn, mx),
            'bwd_xyz': lambda: ops.vm_bwd_xyz(g_feat, planes, vlines, xyz, mn, mx),
            'torch_ops': torch_ops,
            'density_fwd': lambda: ops.vm_density_fwd(planes, vlines, xyz, mn, mx),
            'density_bwd_xyz': lambda: ops.vm_density_bwd_xyz(g_dens, planes, vlines, xyz, mn, mx),
            'density_torch_ops': density_torch_ops}
diffs = {}
for pre in ('', 'density_'):
    got, ref = variants[pre + 'bwd_xyz'](), variants[pre + 'torch_ops']()
    diffs[pre + 'max_diff_to_torch_ops_over_max'] = float((got - ref).abs().max() / ref.abs().max())
    diffs[pre + 'median_diff_to_torch_ops_over_max'] = float((got - ref).abs().median() / ref.abs().max())
    assert torch.equal(got, variants[pre + 'bwd_xyz']())               # bitwise repeatable
    del got, ref
for fn in variants.values():
    series(fn, 2)
TV = {v: [] for v in variants}
for _ in range(args.rounds):
    for v, fn in variants.items():
        TV[v].append(series(fn, args.reps))
row = {'scene': 'roofline_scene', 'rays': args.rays, 'M': M, 'R': R, 'planes': [SIDE, SIDE], 'lines': SIDE, 'layout': 'channels_last',
       'reps': args.reps, 'rounds': args.rounds, 'texel_bytes_gathered': M * 3 * R * 6 * 4, **diffs}
for v in variants:
    row[v] = summary(TV[v])
for pre in ('', 'density_'):
    row[pre + 'bwd_xyz_over_fwd'] = round(row[pre + 'bwd_xyz']['median_ms'] / row[pre + 'fwd']['median_ms'], 3)
    row[pre + 'torch_ops_over_bwd_xyz'] = round(row[pre + 'torch_ops']['median_ms'] / row[pre + 'bwd_xyz']['median_ms'], 3)
emit(row)
del variants, g_feat, g_dens
torch.cuda.empty_cache()

if args.pose:
    from directvoxgo_amd.pose import CameraRefiner
    from directvoxgo_amd.train import render_loss
    sc = synthetic_scene(world=WORLD, n_rays=args.rays, device='cuda')
    rk = dict(near=sc['near'], far=sc['far'], bg=1, stepsize=sc['stepsize'])
    n, S = 24, 128
    poses = torch.stack([pose_spherical(15.0 * i, -30.0, 4.0)[:3, :4] for i in range(n)])
    K = np.array([[1.39 * S, 0, 0.5 * S], [0, 1.39 * S, 0.5 * S], [0, 0, 1]], np.float32)       # lego's field of view
    refiner = CameraRefiner(poses, np.array([[S, S]] * n), np.stack([K] * n)).cuda()
    opt = torch.optim.Adam([refiner.delta], lr=1e-5)                 # (the poses stay what they are over the run)
    cpu = torch.Generator().manual_seed(7)
    view = torch.randint(n, (args.rays,), generator=cpu).cuda()
    pix_i = torch.randint(S, (args.rays,), generator=cpu).cuda()
    pix_j = torch.randint(S, (args.rays,), generator=cpu).cuda()
    target = torch.rand((args.rays, 3), generator=cpu).cuda()
    cfg = dict(TENSORF_FINE_TRAIN, weight_entropy_last=0.0, weight_rgbper=0.0)
    row = {'pose_iteration': {}, 'rays': args.rays, 'views': n, 'side': S, 'world': WORLD, 'R': R, 'reps': args.reps, 'rounds': args.rounds}

    def bump(k, centre, width=0.45):
        return torch.exp(-((torch.linspace(-1, 1, k, device='cuda') - centre) / width) ** 2)

    for cls in (VMTriPlaneVoxGO, TensoRFVoxGO):
        torch.manual_seed(0)
        extra = dict(density_n_comp=R) if cls is TensoRFVoxGO else {}
        model = cls(sc['xyz_min'], sc['xyz_max'], raygrad=True, n_comp=R, **extra, **BASE).cuda()
        with torch.no_grad():
            if cls is VMTriPlaneVoxGO:
                model.density.copy_(sc['density']); model.mask_cache.mask.copy_(sc['mask'])
            else:                                # separable bumps plus a negative constant, as in tests/vm_render_oracle.py
                for i, k in enumerate(PLANE_KEYS):
                    p, ln = model.density_planes[k], model.density_lines[k]
                    p.mul_(0.5); ln.mul_(0.5)
                    c = 0.25 * (i - 1)
                    p[0, 0] = 3.0 * bump(p.shape[2], c)[:, None] * bump(p.shape[3], -c)[None, :]
                    ln[0, 0, :, 0] = 3.0 * bump(ln.shape[2], 0.1 * i)
                    p[0, 1] = 1.0
                    ln[0, 1] = -1.0
                model.mask_cache.mask.fill_(True)
            for q in list(model.planes.values()) + list(model.lines.values()):
                q.normal_(0, 0.5)
        for q in model.parameters():
            q.requires_grad_(False)
        kept = []

        def iteration():
            rays_o, rays_d, viewdirs = refiner.rays(view, pix_i, pix_j)
            out = model(rays_o, rays_d, viewdirs, global_step=None, **rk)
            loss = render_loss(out, target, args.rays, cfg)
            opt.zero_grad(set_to_none=True)
            loss.backward(inputs=[refiner.delta])
            opt.step()
            kept.append(int(out['ray_id'].shape[0]))

        series(iteration, 3)
        rounds = [series(iteration, args.reps) for _ in range(args.rounds)]
        row['pose_iteration'][cls.__name__] = dict(summary(rounds), kept_samples=kept[-1])
        del model
        torch.cuda.empty_cache()
    emit(row)

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        for ln in lines:
            fh.write(json.dumps(ln) + '\n')
