"""CPU check behind the recovery test of tests/test_gpu_vm_raygrad.py: from that test's perturbed poses, Adam on float64
torch.autograd of the ray-differentiable render of VMTriPlaneVoxGO ('vm') or TensoRFVoxGO ('tensorf') restated in torch ops
(tests/vm_render_oracle.py) descends, and every view's pose error shrinks.  No kernel runs: the kept samples come from the CPU oracle's sampler and occupancy lookup,
the two weight filters from a no-grad pass of the same restatement, the targets from the restatement at the true poses.  It
says which capture, perturbation and learning rate the GPU test may use; it proves nothing about the kernels.

  python tools/vm_raygrad_descent_cpu.py --model vm|tensorf [--world 32] [--side 24] [--focal 30] [--views 6] [--rot 2.0] [--shift 0.03]
                                           [--lrate 4e-3] [--iters 200] [--seed 5] [--capture-seed 7]
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

ap = argparse.ArgumentParser()
ap.add_argument('--model', choices=['vm', 'tensorf'], required=True)
ap.add_argument('--world', type=int, default=32)
ap.add_argument('--side', type=int, default=24)
ap.add_argument('--focal', type=float, default=30.0)
ap.add_argument('--views', type=int, default=6)
ap.add_argument('--rot', type=float, default=2.0, help='degrees every pose is turned by')
ap.add_argument('--shift', type=float, default=0.03, help='fraction of the radius every camera is moved by')
ap.add_argument('--lrate', type=float, default=4e-3)
ap.add_argument('--iters', type=int, default=200)
ap.add_argument('--seed', type=int, default=5, help='of the model')
ap.add_argument('--capture-seed', type=int, default=7)
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

import hash_render_oracle as HR  # noqa: E402
import vm_render_oracle as VRO  # noqa: E402
from directvoxgo_amd.pose import CameraRefiner  # noqa: E402

RK = dict(near=2.0, far=6.0, stepsize=0.5, bg=1)
S, NV = args.side, args.views
m = VRO.make_model(args.model, args.world, args.seed)
true, noisy, HWs, Ks = HR.capture(NV, S, args.focal, seed=args.capture_seed, rot_deg=args.rot, shift=args.shift)
view = torch.arange(NV).repeat_interleave(S * S)
pix = torch.arange(S * S).repeat(NV)


def render(ref):
    o, d, v = ref.rays(view, pix % S, pix // S)
    rec = VRO.cpu_record(m, o, d, RK)
    return VRO.restate(m, o, d, v, rec, torch.float64, RK)


with torch.no_grad():
    target = render(CameraRefiner(true, HWs, Ks).double())
print(f'target std {float(target.std()):.4f}')
ref = CameraRefiner(noisy, HWs, Ks).double()
rot0, tr0 = HR.pose_errors(ref.poses(), true)
opt = torch.optim.Adam([ref.delta], lr=args.lrate)
losses = []
for it in range(args.iters):
    loss = (render(ref) - target).pow(2).mean()
    opt.zero_grad()
    loss.backward()
    opt.step()
    losses.append(float(loss.detach()))
rot1, tr1 = HR.pose_errors(ref.poses(), true)
print(f'{args.model}: world {args.world}, model seed {args.seed}, {NV} views of {S} x {S}, focal {args.focal}, capture seed {args.capture_seed}, '
      f'rotation {args.rot} deg, shift {args.shift}, lrate {args.lrate}, {args.iters} iterations')
print(f'loss {losses[0]:.4g} -> {losses[-1]:.4g}')
print('rotation error (deg)', np.degrees(rot0.numpy()).round(3).tolist(), '->', np.degrees(rot1.numpy()).round(3).tolist())
print('translation error', tr0.numpy().round(4).tolist(), '->', tr1.numpy().round(4).tolist())
print('every view improves:', bool((rot1 < rot0).all() and (tr1 < tr0).all()), ' loss descends:', losses[-1] < losses[0])
