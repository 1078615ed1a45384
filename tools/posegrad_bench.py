"""What one joint pose-and-model iteration costs, eager against fused, on the two 160^3 scenes of
bench.py: the lego-like sparse scene (scenes.synthetic_scene) and the roofline scene (scenes.roofline_scene), 8192 rays, the
128-wide fused colour head, FINE_TRAIN with masked Adam on both grids.

Four things are timed, alternating within a round, in one process, each on its own copy of the model:
  a  eager   the iteration of pose.refine_poses(train_model=True): rays from the pose -> DirectVoxGO._forward_raygrad (the
             op-by-op sequence) -> train.render_loss -> backward -> MaskedAdam.step on dense gradients -> Adam on the pose
  b  fused   the iteration of pose.refine_poses(train_model=True, fused=True): rays from the pose -> train.TrainStep (fused
             march, dvgo_march_ray_bwd first in the backward, brick scatter with Adam inside) -> Adam on the pose
  c  plain   the TrainStep call of b on the same rays detached: what the step costs without the ray gradient
  d  leaf    the TrainStep call of b on the same rays as leaves that require grad: c plus dvgo_march_ray_bwd and nothing of
             the pose (no torch graph from a parameter to the rays, no optimizer on it), so d - c is the ray gradient's own
             cost and b - d what the pose's torch graph and its Adam add on the host
The loop bodies are pose.refine_poses's, restated here so that one iteration can be timed.  The scenes come with rays, not
with cameras, so the pose is one se(3) correction of the whole batch (pose.se3_exp of a [1,6] parameter applied to the scene's
rays): the torch graph from the parameter to the rays is the size a CameraRefiner's is, and it is the same in a and b.
Learning rates are 1e-5 of FINE_TRAIN's so that the scene the windows see stays the scene that was built.

A sample is one device-event pair around `reps` back-to-back iterations, `reps` chosen after the warm-up so that a window is
at least `--window` seconds; reported per iteration: the median over the rounds and the spread (max - min).  One JSON line
per scene; `--out FILE` also writes them there.  `--variants` restricts what runs (the kernel-trace run of the fused
iteration alone: rocprofv3 --kernel-trace --stats -- python tools/posegrad_bench.py --variants b --rounds 1 --window 0.2).

  python tools/posegrad_bench.py [--rounds 3] [--window 1.0] [--scenes lego,roofline] [--variants abcd] [--out FILE]
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--window', type=float, default=1.0, help='seconds per timed sample, at least')
ap.add_argument('--world', type=int, default=160)
ap.add_argument('--rays', type=int, default=8192)
ap.add_argument('--scenes', default='lego,roofline')
ap.add_argument('--variants', default='abcd')
ap.add_argument('--out', default=None)
args = ap.parse_args()

import torch  # noqa: E402

from directvoxgo_amd.dvgo import DirectVoxGO  # noqa: E402
from directvoxgo_amd.pose import se3_exp  # noqa: E402
from directvoxgo_amd.scenes import roofline_scene, synthetic_scene  # noqa: E402
from directvoxgo_amd.train import FINE_TRAIN, TrainStep, create_optimizer_or_freeze_model, render_loss  # noqa: E402

assert torch.cuda.is_available(), 'posegrad_bench needs the GPU: a CPU run measures nothing'
CFG = dict(FINE_TRAIN, lrate_density=1e-6, lrate_k0=1e-6, lrate_rgbnet=1e-8)
LRATE_POSE = 1e-7


def build(sc):
    torch.manual_seed(777)
    m = DirectVoxGO(sc['xyz_min'], sc['xyz_max'], num_voxels=args.world ** 3, num_voxels_base=args.world ** 3, alpha_init=1e-2,
                    fast_color_thres=1e-4, rgbnet_dim=12, rgbnet_width=128, rgbnet_direct=True).cuda()
    with torch.no_grad():
        m.density.copy_(sc['density']); m.k0.copy_(sc['k0']); m.mask_cache.mask.copy_(sc['mask'])
    return m


class Pose(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.delta = torch.nn.Parameter(torch.zeros(1, 6, device='cuda'))

    def rays(self, o, d):
        T = se3_exp(self.delta)[0]
        rd = d @ T[:, :3].t()
        return (o @ T[:, :3].t() + T[:, 3]).contiguous(), rd.contiguous(), (rd / rd.norm(dim=-1, keepdim=True)).detach().contiguous()


def make_iterations(sc):
    rk = dict(near=sc['near'], far=sc['far'], bg=1, stepsize=sc['stepsize'])
    o, d, v, target = sc['rays_o'], sc['rays_d'], sc['viewdirs'], sc['target']
    its, info = {}, {}
    if 'a' in args.variants:
        ma, pa = build(sc), Pose()
        opt_pose_a = torch.optim.Adam([pa.delta], lr=LRATE_POSE)
        opt_model = create_optimizer_or_freeze_model(ma, CFG, 0)

        def eager():
            ro, rd, vd = pa.rays(o, d)
            res = ma(ro, rd, vd, global_step=None, **rk)
            loss = render_loss(res, target, ro.shape[0], CFG)
            opt_pose_a.zero_grad(set_to_none=True)
            opt_model.zero_grad(set_to_none=True)
            loss.backward()
            opt_model.step()
            opt_pose_a.step()
            info['samples'] = res['weights'].shape[0]
        its['a'] = eager
    if 'b' in args.variants:
        mb, pb = build(sc), Pose()
        mb.fused_raygrad = True
        opt_pose_b = torch.optim.Adam([pb.delta], lr=LRATE_POSE)
        step_b = TrainStep(mb, CFG, rk)
        n = [0]

        def fused():
            ro, rd, vd = pb.rays(o, d)
            opt_pose_b.zero_grad(set_to_none=True)
            n[0] += 1
            step_b(ro, rd, vd, target, n[0])
            opt_pose_b.step()
            info['fused_adam'] = step_b.last_fused_adam
        its['b'] = fused
    if 'c' in args.variants:
        mc = build(sc)
        step_c = TrainStep(mc, CFG, rk)
        k = [0]

        def plain():
            k[0] += 1
            step_c(o, d, v, target, k[0])
        its['c'] = plain
    if 'd' in args.variants:
        md = build(sc)
        md.fused_raygrad = True
        step_d = TrainStep(md, CFG, rk)
        j = [0]

        def leaf():
            j[0] += 1
            ro, rd = o.detach().requires_grad_(), d.detach().requires_grad_()
            step_d(ro, rd, v, target, j[0])
        its['d'] = leaf
    return its, info


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


lines = []
for name in args.scenes.split(','):
    mk = {'lego': synthetic_scene, 'roofline': roofline_scene}[name]
    sc = mk(world=args.world, n_rays=args.rays, seed=777, device='cuda')
    its, info = make_iterations(sc)
    reps = {}
    for key, fn in its.items():                                  # warm-up, then the repetitions of a window
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        reps[key] = max(3, math.ceil(args.window * 1e3 / timed(fn, 5)))
    t = {key: [] for key in its}
    for _ in range(args.rounds):
        for key, fn in its.items():
            t[key].append(timed(fn, reps[key]))
    rec = {'scene': name, 'world': args.world, 'rays': args.rays, 'rounds': args.rounds, 'window_s': args.window, **info}
    for key, label in (('a', 'eager'), ('b', 'fused'), ('c', 'plain'), ('d', 'leaf')):
        if key in t:
            rec[f'{label}_ms'] = round(median(t[key]), 4)
            rec[f'{label}_spread_ms'] = round(max(t[key]) - min(t[key]), 4)
            rec[f'{label}_reps'] = reps[key]
    if 'a' in t and 'b' in t:
        rec['eager_over_fused'] = round(median(t['a']) / median(t['b']), 3)
    if 'b' in t and 'c' in t:
        rec['fused_minus_plain_ms'] = round(median(t['b']) - median(t['c']), 4)
    if 'd' in t and 'c' in t:
        rec['leaf_minus_plain_ms'] = round(median(t['d']) - median(t['c']), 4)
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)
    del its, sc
    torch.cuda.empty_cache()
if args.out:
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
