"""Cost of the hash sampler's position gradient (csrc/hash_xyz.hip, dvgo_hash_bwd_xyz) beside the forward that moves the same
rows (dvgo_hash_fwd), and beside the same derivative restated in torch ops -- integer index arithmetic, row gathers, autograd:
what a user would write without the kernel.

Positions come from real marches, in ray order: the 8192 x 256 = 2 097 152 samples of scenes.roofline_scene and the kept
samples of the sparse scenes.synthetic_scene, both at 160^3.  Tables: L = 16, F = 2 and L = 8, F = 4, 2^19 rows per hashed
level, base 16, finest 512, values N(0, 0.5).  One lane mapping was built (one lane per sample, the levels in a loop:
csrc/hash_xyz.hip says why), so there is no A/B of mappings.  One process, every variant warmed up, the variants alternating
within a round, device events around each call, the median over rounds x reps and the spread (max - min of the per-round
medians) per variant:
  fwd         ops.hash_fwd
  bwd_xyz     ops.hash_bwd_xyz (its output allocation included)
  torch_ops   forward of the restatement plus torch.autograd.grad with respect to the positions
The kernel's result is compared with the restatement's first (largest difference over the largest gradient).
`--pose`: one pose.refine_poses iteration (without train_model) of a HashVoxGO(raygrad=True) at --rays random pixels of 24 views
of the synthetic scene: CameraRefiner.rays -> model -> train.render_loss -> backward into delta -> Adam on delta.
Prints one JSON line per case; `--out FILE` also writes them there.

  python tools/hash_raygrad_bench.py [--reps 10] [--rounds 3] [--rays 8192] [--pose] [--out FILE]
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
ap.add_argument('--pose', action='store_true', help='also time one refine_poses iteration')
ap.add_argument('--out', default=None)
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from directvoxgo_amd import ops  # noqa: E402
from directvoxgo_amd.fused import fused_march  # noqa: E402
from directvoxgo_amd.hashgrid import HASH_FINE_TRAIN, HashVoxGO, hash_levels  # noqa: E402
from directvoxgo_amd.scenes import pose_spherical, roofline_scene, synthetic_scene  # noqa: E402

assert torch.cuda.is_available(), 'hash_raygrad_bench needs the GPU: a CPU run measures nothing'
TABLES = [dict(n_levels=16, n_feat=2), dict(n_levels=8, n_feat=4)]
WORLD = 160
BASE = dict(num_voxels=WORLD ** 3, num_voxels_base=WORLD ** 3, alpha_init=1e-2, fast_color_thres=1e-4)
PRIMES = (1, 2654435761, 805459861)


def positions(sc):
    """The kept samples of the scene's rays, from the fused march, in ray order."""
    m = HashVoxGO(sc['xyz_min'], sc['xyz_max'], n_levels=2, log2_hashmap_size=4, **BASE).cuda()
    with torch.no_grad():
        m.density.copy_(sc['density']); m.mask_cache.mask.copy_(sc['mask'])
        cfg = m._march_cfg(sc['near'], sc['far'], sc['stepsize'])
        pts = fused_march(m.density, m.density.detach()[:, :0], sc['rays_o'], sc['rays_d'], cfg, positions=True)[3]
    return pts.contiguous(), m.xyz_min.clone(), m.xyz_max.clone()


def torch_features(table, xyz, mn, mx, lv):
    """ops.hash_sample in torch ops, differentiable in xyz: the coordinate clamped into the lattice, the floor node detached,
    rows by integer arithmetic (int64 products and a mask below 2^32 give the wrapping 32-bit hash), eight row gathers."""
    out = []
    for l in range(lv.L):
        R = torch.tensor(lv.res[l], dtype=torch.float32, device=xyz.device)
        g = ((((xyz - mn) / (mx - mn)) * 2 - 1) + 1) / 2 * (R - 1)
        g = torch.where((g >= 0) & (g <= R - 1), g, g.detach().clamp_min(0).minimum(R - 1))      # (no gradient where the clamp acts)
        f = torch.minimum(g.detach().floor(), R - 2)
        w = torch.stack([(f + 1) - g, g - f], -1)                                 # [M,3,2]
        fi = f.long()
        size = lv.offsets[l + 1] - lv.offsets[l]
        acc = 0
        for n in range(8):
            b = ((n >> 2) & 1, (n >> 1) & 1, n & 1)
            ix, iy, iz = (fi[:, a] + b[a] for a in range(3))
            if lv.hashed[l]:
                row = ((ix * PRIMES[0]) ^ (iy * PRIMES[1]) ^ (iz * PRIMES[2])) & (size - 1)
            else:
                row = (ix * lv.res[l][1] + iy) * lv.res[l][2] + iz
            wn = (w[:, 0, b[0]] * w[:, 1, b[1]]) * w[:, 2, b[2]]
            acc = acc + wn[:, None] * table[lv.offsets[l] + row]
        out.append(acc)
    return torch.cat(out, -1)


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
scenes = {'roofline_scene': roofline_scene(world=WORLD, n_rays=args.rays, device='cuda'),
          'synthetic_scene': synthetic_scene(world=WORLD, n_rays=args.rays, device='cuda')}
for name, sc in scenes.items():
    xyz, mn, mx = positions(sc)
    M = xyz.shape[0]
    for T in TABLES:
        L, Fc = T['n_levels'], T['n_feat']
        res, off = hash_levels(mn, mx, L, 16, 512, 19)
        lv = ops.HashLevels(res, off)
        table = torch.randn(lv.rows, Fc, generator=gen, device='cuda') * 0.5
        gout = torch.randn((M, L * Fc), generator=gen, device='cuda')

        def torch_ops():
            x = xyz.clone().requires_grad_()
            return torch.autograd.grad(torch_features(table, x, mn, mx, lv), x, gout)[0]

        variants = {'fwd': lambda: ops.hash_fwd(table, xyz, mn, mx, lv),
                    'bwd_xyz': lambda: ops.hash_bwd_xyz(table, gout, xyz, mn, mx, lv),
                    'torch_ops': torch_ops}
        got, ref = variants['bwd_xyz'](), variants['torch_ops']()
        diff = float((got - ref).abs().max() / ref.abs().max())
        assert torch.equal(got, variants['bwd_xyz']())                 # bitwise repeatable
        del got, ref
        for fn in variants.values():
            series(fn, 2)
        TV = {v: [] for v in variants}
        for _ in range(args.rounds):
            for v, fn in variants.items():
                TV[v].append(series(fn, args.reps))
        row = {'scene': name, 'rays': args.rays, 'M': M, 'L': L, 'F': Fc, 'table_rows': lv.rows, 'dense_levels': lv.hashed.count(False),
               'table_MB': round(lv.rows * Fc * 4 / 2 ** 20, 1), 'reps': args.reps, 'rounds': args.rounds,
               'max_diff_to_torch_ops_over_max': diff, 'row_bytes_gathered': M * L * 8 * Fc * 4}
        for v in variants:
            row[v] = summary(TV[v])
        row['bwd_xyz_over_fwd'] = round(row['bwd_xyz']['median_ms'] / row['fwd']['median_ms'], 3)
        row['torch_ops_over_bwd_xyz'] = round(row['torch_ops']['median_ms'] / row['bwd_xyz']['median_ms'], 3)
        emit(row)
        del table, gout, variants
        torch.cuda.empty_cache()

if args.pose:
    from directvoxgo_amd.pose import CameraRefiner
    from directvoxgo_amd.train import render_loss
    sc = scenes['synthetic_scene']
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
    cfg = dict(HASH_FINE_TRAIN, weight_entropy_last=0.0, weight_rgbper=0.0)
    row = {'pose_iteration': {}, 'rays': args.rays, 'views': n, 'side': S, 'world': WORLD, 'reps': args.reps, 'rounds': args.rounds}
    for T in TABLES:
        torch.manual_seed(0)
        model = HashVoxGO(sc['xyz_min'], sc['xyz_max'], raygrad=True, **T, **BASE).cuda()
        with torch.no_grad():
            model.density.copy_(sc['density']); model.mask_cache.mask.copy_(sc['mask'])
            model.hash_table.normal_(0, 0.5)
        for p in model.parameters():
            p.requires_grad_(False)
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
        row['pose_iteration'][f"HashVoxGO_L{T['n_levels']}_F{T['n_feat']}"] = dict(summary(rounds), kept_samples=kept[-1])
        del model
        torch.cuda.empty_cache()
    emit(row)

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        for ln in lines:
            fh.write(json.dumps(ln) + '\n')
