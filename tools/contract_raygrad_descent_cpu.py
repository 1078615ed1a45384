"""CPU check behind the recovery test of tests/test_gpu_contract_raygrad.py: from that test's perturbed poses, Adam on float64
torch.autograd of the render restated in torch ops (tests/contract_render_oracle.py) descends, and every view's pose error
shrinks.  No kernel runs: the kept samples come from the numpy sampler of tests/unbounded_oracle.py, the early stop from a
no-grad pass of the same restatement, the targets from the restatement at the true poses.  It says which perturbation and
learning rate the GPU test may use; it proves nothing about the kernels.

  python tools/contract_raygrad_descent_cpu.py [--world 32] [--side 16] [--views 6] [--rot 1.0] [--shift 0.03] [--lrate 1e-3] [--iters 200]
"""
import argparse
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

ap = argparse.ArgumentParser()
ap.add_argument('--world', type=int, default=32)
ap.add_argument('--side', type=int, default=16)
ap.add_argument('--views', type=int, default=6)
ap.add_argument('--rot', type=float, default=1.0, help='degrees every pose is turned by')
ap.add_argument('--shift', type=float, default=0.03, help='distance every camera is moved by')
ap.add_argument('--lrate', type=float, default=1e-3)
ap.add_argument('--iters', type=int, default=200)
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

import contract_render_oracle as R  # noqa: E402
import unbounded_oracle as U  # noqa: E402
from directvoxgo_amd import scenes  # noqa: E402
from directvoxgo_amd.pose import CameraRefiner, se3_exp  # noqa: E402

B, STEP, BG, S, NV = 0.2, 0.5, 0.5, args.side, args.views
b32 = float(np.float32(B))
gen = torch.Generator().manual_seed(777)                        # scenes.unbounded_scene's grids and cameras, in its order
density, k0 = scenes.unbounded_grids(args.world, B, gen)
true = scenes.unbounded_cameras(NV, gen)[:, :3, :4]
g2 = torch.Generator().manual_seed(7)                           # the GPU test's perturbation
axis = torch.randn(NV, 3, generator=g2)
axis = axis / axis.norm(dim=-1, keepdim=True)
shift = torch.randn(NV, 3, generator=g2)
shift = shift / shift.norm(dim=-1, keepdim=True) * args.shift
E = se3_exp(torch.cat([axis * math.radians(args.rot), torch.zeros(NV, 3)], -1))[:, :, :3]
noisy = torch.cat([E @ true[:, :, :3], true[:, :, 3:] + shift[:, :, None]], -1)
focal = 0.75 * S
K = np.array([[focal, 0, 0.5 * S], [0, focal, 0.5 * S], [0, 0, 1]], np.float32)
HWs, Ks = np.array([[S, S]] * NV), np.stack([K] * NV)
t_tab = torch.tensor(U.t_table(args.world, STEP, B)[0], dtype=torch.float64)
c, r = torch.zeros(3, dtype=torch.float64), torch.ones(3, dtype=torch.float64)
act_shift = math.log(1 / (1 - 1e-2) - 1)
D, K0 = density[0, 0].double(), k0[0].double()
view = torch.arange(NV).repeat_interleave(S * S)
pix = torch.arange(S * S).repeat(NV)


def render(ref):
    o, d, _ = ref.rays(view, pix % S, pix // S)
    _, rid, sid, _, _ = U.sample(o.detach().numpy(), d.detach().numpy(), [0, 0, 0], [1, 1, 1], args.world, STEP, B, 'inf')
    rid, sid = torch.tensor(rid), torch.tensor(sid)
    with torch.no_grad():                                       # the early stop: samples behind the first T < 1e-3
        q = R.contract(o.detach(), d.detach(), c, r, t_tab, b32, 'inf')[rid, sid]
        a = 1 - (1 + torch.exp(R._sample(D[None], q, 1 + b32)[:, 0] + act_shift)) ** (-STEP)
        Ta = torch.cumprod(torch.ones((o.shape[0], len(t_tab)), dtype=torch.float64).index_put((rid, sid), 1 - a + 1e-10), 1)
        Tb = torch.cat([torch.ones((o.shape[0], 1), dtype=torch.float64), Ta[:, :-1]], 1)
        stop_after = Tb[rid, sid] < 1e-3
    return R.render(o, d, rid, sid, t_tab, c, r, b32, 'inf', D, K0, act_shift, STEP, BG, stop_after=stop_after)['rgb_marched']


def errors(est):
    est, tr = est.detach().double(), true.double()
    rel = est[:, :, :3] @ tr[:, :, :3].transpose(1, 2)
    cos = ((rel.diagonal(dim1=1, dim2=2).sum(-1) - 1) / 2).clamp(-1, 1)
    return torch.acos(cos), (est[:, :, 3] - tr[:, :, 3]).norm(dim=-1)


with torch.no_grad():
    target = render(CameraRefiner(true, HWs, Ks).double())
ref = CameraRefiner(noisy, HWs, Ks).double()
rot0, tr0 = errors(ref.poses())
opt = torch.optim.Adam([ref.delta], lr=args.lrate)
losses = []
for it in range(args.iters):
    loss = (render(ref) - target).pow(2).mean()
    opt.zero_grad()
    loss.backward()
    opt.step()
    losses.append(float(loss.detach()))
rot1, tr1 = errors(ref.poses())
print(f'world {args.world}, {NV} views of {S} x {S}, rotation {args.rot} deg, shift {args.shift}, lrate {args.lrate}, {args.iters} iterations')
print(f'loss {losses[0]:.4g} -> {losses[-1]:.4g}')
print('rotation error (deg)', np.degrees(rot0.numpy()).round(3).tolist(), '->', np.degrees(rot1.numpy()).round(3).tolist())
print('translation error', tr0.numpy().round(4).tolist(), '->', tr1.numpy().round(4).tolist())
print('every view improves:', bool((rot1 < rot0).all() and (tr1 < tr0).all()), ' loss descends:', losses[-1] < losses[0])
