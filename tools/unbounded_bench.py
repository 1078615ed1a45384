"""Speed of the contracted model's training step (directvoxgo_amd.dcvgo) on an unbounded scene: a DirectContractedVoxGO
at --world^3 with the 12-channel feature grid and the HIP colour head, density and features of a trained-looking scene
(scenes.unbounded_grids), --rays rays per step from cameras inside the foreground box, weight_distortion = 0.01.
Times, with device events after a warm-up, the whole TrainStep and, separately, the contracted sampler and the
distortion loss on the step's samples.  Prints one JSON line.

  python tools/unbounded_bench.py [--world 160] [--rays 8192] [--steps 20]
  rocprofv3 --kernel-trace --stats -d DIR -o ub -- python tools/unbounded_bench.py --steps 20
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from directvoxgo_amd import scenes  # noqa: E402
from directvoxgo_amd.dcvgo import DirectContractedVoxGO  # noqa: E402
from directvoxgo_amd.distortion import distortion_loss  # noqa: E402
from directvoxgo_amd.train import TrainStep  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--world', type=int, default=160)
ap.add_argument('--rays', type=int, default=8192)
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=3)
args = ap.parse_args()

gen = torch.Generator().manual_seed(0)
W = args.world
m = DirectContractedVoxGO([-1, -1, -1], [1, 1, 1], num_voxels=W ** 3, num_voxels_base=W ** 3, alpha_init=1e-2,
                          fast_color_thres=1e-4, rgbnet_dim=12, rgbnet_direct=True).cuda()
density, k0 = scenes.unbounded_grids(W, 0.2, gen)
with torch.no_grad():
    m.density.copy_(density.cuda())
    m.k0.copy_((torch.randn(m.k0.shape, generator=gen) * 0.3).cuda())
poses = scenes.unbounded_cameras(16, gen)
rays = [scenes.camera_rays(64, 64, 48.0, c2w) for c2w in poses]
ro, rd, vd = (torch.cat([r[i] for r in rays]).cuda().contiguous() for i in range(3))
target = torch.rand(ro.shape, generator=gen).cuda()
cfg = dict(N_iters=args.steps, N_rand=args.rays, lrate_density=1e-1, lrate_k0=1e-1, lrate_rgbnet=1e-3, lrate_decay=20,
           pervoxel_lr=False, weight_main=1.0, weight_entropy_last=0.001, weight_rgbper=0.01, tv_every=1, tv_after=0,
           tv_before=0, tv_dense_before=0, weight_tv_density=0.0, weight_tv_k0=0.0, pg_scale=[],
           skip_zero_grad_fields=['density', 'k0'], weight_distortion=0.01)
rk = dict(near=0, far=1e4, stepsize=0.5, bg=0.5)
step = TrainStep(m, cfg, rk)
batches = [torch.randint(ro.shape[0], (args.rays,), generator=gen).cuda() for _ in range(args.steps + args.warmup)]


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


for i in range(args.warmup):
    s = batches[i]
    step(ro[s], rd[s], vd[s], target[s], i + 1)
ms_step = timed(lambda i: step(ro[batches[i]], rd[batches[i]], vd[batches[i]], target[batches[i]], i + 1), args.steps)
s = batches[0]
ms_sample = timed(lambda i: m.sample_ray(ro[s], rd[s], 0.5), args.steps)
res = m(ro[s], rd[s], vd[s], **rk)
w = res['weights'].detach().requires_grad_(True)
ms_dist = timed(lambda i: distortion_loss(w, res['s'], res['n_max'], res['ray_id'], args.rays), args.steps)
print(json.dumps({'world': W, 'rays': args.rays, 'n_max': res['n_max'], 'samples': int(res['weights'].shape[0]),
                  'step_ms': round(ms_step, 4), 'sampler_ms': round(ms_sample, 4), 'distortion_ms': round(ms_dist, 4)}))
