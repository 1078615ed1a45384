"""Synthetic inputs for tests, smoke and bench (no dataset exists in the image).

Follows SURVEY.md section 8d:
  * lego-like cameras: pose_spherical(theta ~ U(-180,180), phi = -30, r = 4) and pixel-centre pinhole
    rays (conventions of /root/reference/lib/load_blender.py:14-42 and lib/ray_utils.py:9-47,80-85;
    pinned against the reference run in tests/golden/rays.npz);
  * a smooth blob density field with low-passed noise, random features, occupancy mask from the
    max-pooled activated density;
  * the "roofline case": unit-direction rays crossing the box face to face with near = 0 and
    far = 255.5 * stepdist, so that every ray has exactly 256 in-box samples, a density for which no
    sample is culled by either threshold and no ray terminates early (M = N * 256).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F


def pose_spherical(theta, phi, radius):
    """camera-to-world of a camera on a sphere looking at the origin (blender convention)."""
    th, ph = math.radians(theta), math.radians(phi)
    trans = torch.tensor([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, radius], [0, 0, 0, 1]], dtype=torch.float32)
    rphi = torch.tensor([[1, 0, 0, 0], [0, math.cos(ph), -math.sin(ph), 0], [0, math.sin(ph), math.cos(ph), 0],
                         [0, 0, 0, 1]], dtype=torch.float32)
    rth = torch.tensor([[math.cos(th), 0, -math.sin(th), 0], [0, 1, 0, 0], [math.sin(th), 0, math.cos(th), 0],
                        [0, 0, 0, 1]], dtype=torch.float32)
    flip = torch.tensor([[-1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], dtype=torch.float32)
    return flip @ (rth @ (rphi @ trans))


def camera_rays(H, W, focal, c2w, pix_i=None, pix_j=None):
    """Pixel-centre pinhole rays (non-inverse-y convention): returns rays_o, rays_d, viewdirs for
    the given pixel columns/rows (all pixels, row-major, when omitted)."""
    if pix_i is None:
        jj, ii = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing='ij')
        pix_i, pix_j = ii.reshape(-1), jj.reshape(-1)
    i = pix_i + 0.5
    j = pix_j + 0.5
    dirs = torch.stack([(i - 0.5 * W) / focal, -(j - 0.5 * H) / focal, -torch.ones_like(i)], -1)
    rays_d = torch.sum(dirs[..., None, :] * c2w[:3, :3], -1)
    rays_o = c2w[:3, 3].expand(rays_d.shape)
    viewdirs = rays_d / rays_d.norm(dim=-1, keepdim=True)
    return rays_o.contiguous(), rays_d.contiguous(), viewdirs.contiguous()


def lego_like_rays(n_rays, gen, n_views=100, H=800, W=800, focal=1111.11, radius=4.0, phi=-30.0):
    """n_rays rays drawn uniformly from the pixels of n_views random lego-like cameras."""
    thetas = torch.rand(n_views, generator=gen) * 360 - 180
    view = torch.randint(n_views, (n_rays,), generator=gen)
    pi = torch.randint(W, (n_rays,), generator=gen).float()
    pj = torch.randint(H, (n_rays,), generator=gen).float()
    ro = torch.empty(n_rays, 3); rd = torch.empty(n_rays, 3); vd = torch.empty(n_rays, 3)
    for v in range(n_views):
        sel = (view == v).nonzero().squeeze(1)
        if sel.numel() == 0:
            continue
        o, d, u = camera_rays(H, W, focal, pose_spherical(float(thetas[v]), phi, radius), pi[sel], pj[sel])
        ro[sel], rd[sel], vd[sel] = o, d, u
    return ro, rd, vd


def blob_density(ws, xyz_min, xyz_max, gen, amp=16.0, bias=-9.0, noise=1.5, radius=0.9):
    ax = [torch.linspace(float(xyz_min[a]), float(xyz_max[a]), ws[a]) for a in range(3)]
    xx, yy, zz = torch.meshgrid(*ax, indexing='ij')
    r = torch.sqrt(xx ** 2 + yy ** 2 + zz ** 2) / radius
    n = torch.randn(ws, generator=gen)
    n = F.avg_pool3d(n[None, None], 3, 1, 1)[0, 0]
    return amp * torch.exp(-r ** 4) + bias + noise * n


def activate(density, act_shift, interval):
    return 1 - torch.exp(-F.softplus(density + act_shift) * interval)


def synthetic_scene(world=160, n_rays=8192, seed=777, device='cpu', k0_dim=12, alpha_init=1e-2,
                    fast_color_thres=1e-4, bbox=1.5, bound_scale=1.05, stepsize=0.5):
    """config-2-like scene (lego fine stage): cubic bbox [-1.5,1.5]^3 * 1.05, world^3 grid, blob density
    with ~15-30 % occupied voxels, N(0, 0.3^2) features, lego-like rays, near/far = 2/6."""
    gen = torch.Generator().manual_seed(seed)
    mn = torch.full((3,), -bbox * bound_scale); mx = torch.full((3,), bbox * bound_scale)
    ws = (world, world, world)
    act_shift = math.log(1 / (1 - alpha_init) - 1)
    density = blob_density(ws, mn, mx, gen)
    k0 = torch.randn((1, k0_dim, *ws), generator=gen) * 0.3
    alpha = F.max_pool3d(activate(density, act_shift, 1.0)[None, None], 3, 1, 1)[0, 0]
    mask = alpha > fast_color_thres
    ro, rd, vd = lego_like_rays(n_rays, gen)
    target = torch.rand((n_rays, 3), generator=gen)
    sc = dict(xyz_min=mn, xyz_max=mx, density=density[None, None], k0=k0, mask=mask, rays_o=ro, rays_d=rd,
              viewdirs=vd, target=target)
    sc = {k: v.to(device) for k, v in sc.items()}
    sc.update(near=2.0, far=6.0, stepsize=stepsize, world=world, occupancy=float(mask.float().mean()))
    return sc


def roofline_rays(n_rays, gen, half):
    """Unit-direction chords from one face of the cube [-half, half]^3 (1e-4 inside) to the opposite
    face, every other coordinate strictly inside: chord length >= 2*half - 2e-4."""
    axis = torch.randint(3, (n_rays,), generator=gen)
    side = torch.randint(2, (n_rays,), generator=gen).float() * 2 - 1
    inset = half * (1 - 2e-3)
    o = (torch.rand((n_rays, 3), generator=gen) * 2 - 1) * inset
    t = (torch.rand((n_rays, 3), generator=gen) * 2 - 1) * inset
    idx = torch.arange(n_rays)
    o[idx, axis] = -side * (half - 1e-4)
    t[idx, axis] = side * (half - 1e-4)
    d = t - o
    d = d / d.norm(dim=-1, keepdim=True)
    return o.contiguous(), d.contiguous()


def roofline_scene(world=160, n_rays=8192, n_samples=256, seed=777, device='cpu', k0_dim=12, bbox=1.5,
                   bound_scale=1.05, stepsize=0.5):
    """The 8192 x 256 roofline case of SURVEY.md section 8d.  Every ray is a unit-direction chord
    from one box face (1e-4 inside) to the opposite face; near = 0, far = (n_samples - 0.5) * stepdist;
    density ~ N(0, 0.1^2) (alpha ~ 0.005 per sample: above the 1e-4 threshold, total opacity far from
    the 1e-3 early-stop), mask all true.  Every ray therefore yields exactly n_samples samples that all
    survive to the feature lookup."""
    gen = torch.Generator().manual_seed(seed)
    half = bbox * bound_scale
    mn = torch.full((3,), -half); mx = torch.full((3,), half)
    ws = (world, world, world)
    voxel_size = ((mx - mn).prod() / world ** 3).pow(1 / 3)
    stepdist = float(stepsize * voxel_size)
    o, d = roofline_rays(n_rays, gen, half)
    far = (n_samples - 0.5) * stepdist
    assert far < 2 * half - 1e-2, 'chord shorter than the sampled span'
    density = torch.randn((1, 1, *ws), generator=gen) * 0.1
    k0 = torch.randn((1, k0_dim, *ws), generator=gen) * 0.3
    mask = torch.ones(ws, dtype=torch.bool)
    target = torch.rand((n_rays, 3), generator=gen)
    sc = dict(xyz_min=mn, xyz_max=mx, density=density, k0=k0, mask=mask, rays_o=o.contiguous(),
              rays_d=d.contiguous(), viewdirs=d.clone().contiguous(), target=target)
    sc = {k: v.to(device) for k, v in sc.items()}
    sc.update(near=0.0, far=far, stepsize=stepsize, world=world, n_samples=n_samples, occupancy=1.0)
    return sc


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """camera-to-world [4,4] of a camera at `eye` looking at `target` (camera looks down its -z axis)."""
    eye, target, up = (torch.as_tensor(v, dtype=torch.float32) for v in (eye, target, up))
    back = eye - target
    back = back / back.norm()
    right = torch.linalg.cross(up, back)
    if float(right.norm()) < 1e-6:
        right = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0]), back)
    right = right / right.norm()
    upv = torch.linalg.cross(back, right)
    c2w = torch.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, upv, back, eye
    return c2w


def unbounded_grids(world, bg_len, gen, blob_r=0.35, shell=(1.06, 1.14)):
    """Ground-truth grids of an unbounded scene in contracted space [-(1+b), 1+b]^3 (max norm): a blob of radius
    `blob_r` around the origin inside the unit box, and an opaque textured background shell at contracted radius
    `shell` (normalised distance 1 / ((1+b) - radius) * b: about 1.4 to 2.5 for b = 0.2).  -> density [1,1,W,W,W] and
    a colour grid k0 [1,3,W,W,W] (pre-sigmoid)."""
    lim = 1 + bg_len
    ax = torch.linspace(-lim, lim, world)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing='ij')
    n = torch.maximum(torch.maximum(x.abs(), y.abs()), z.abs())
    r = torch.sqrt(x ** 2 + y ** 2 + z ** 2)
    noise = F.avg_pool3d(torch.randn((1, 1, world, world, world), generator=gen), 3, 1, 1)[0, 0]
    density = 24 * torch.exp(-(r / blob_r) ** 4) - 12 + noise
    in_shell = (n > shell[0]) & (n < shell[1])
    density = torch.where(in_shell, torch.full_like(density, 12.0), density)
    k0 = torch.stack([
        torch.where(in_shell, 2.5 * torch.sin(9 * x) * torch.cos(7 * y), 3 * x),
        torch.where(in_shell, 2.5 * torch.sin(8 * y + 1) * torch.cos(6 * z), -1 + 2 * z),
        torch.where(in_shell, 2.5 * torch.cos(7 * z + 2) * torch.sin(5 * x), 1 - 3 * y)])
    return density[None, None].contiguous(), k0[None].contiguous()


def unbounded_cameras(n_views, gen, radius=(0.55, 0.85)):
    """Cameras inside the unit foreground box: each at a random direction and distance `radius` from the origin,
    looking inward (at the origin, through the blob to the background behind it) or outward (straight at the
    background), alternately."""
    poses = []
    for v in range(n_views):
        d = torch.randn(3, generator=gen)
        d = d / d.norm()
        rr = radius[0] + (radius[1] - radius[0]) * float(torch.rand(1, generator=gen))
        eye = d * rr
        jitter = torch.randn(3, generator=gen) * 0.1
        target = jitter if v % 2 == 0 else eye + d + jitter
        poses.append(look_at(eye, target))
    return torch.stack(poses)


@torch.no_grad()
def unbounded_scene(world=64, bg_len=0.2, n_train=24, n_test=4, H=32, W=32, focal=24.0, seed=777, stepsize=0.5,
                    bg=0.5, device='cuda'):
    """An unbounded test scene: ground-truth grids (`unbounded_grids`), cameras inside the foreground box [-1, 1]^3
    looking inward and outward (`unbounded_cameras`), and targets rendered from the ground truth by
    DirectContractedVoxGO itself (its forward is pinned against tests/unbounded_oracle.py).  Returns the ground-truth
    model, flat training rays / targets, and the held-out views as (poses, HW, Ks, images) for evaluate_viewpoints."""
    from .dcvgo import DirectContractedVoxGO
    gen = torch.Generator().manual_seed(seed)
    density, k0 = unbounded_grids(world, bg_len, gen)
    gt = DirectContractedVoxGO([-1, -1, -1], [1, 1, 1], num_voxels=world ** 3, num_voxels_base=world ** 3, alpha_init=1e-2,
                               bg_len=bg_len).to(device)
    gt.density.data.copy_(density)
    gt.k0.data.copy_(k0)
    render_kwargs = dict(near=0.0, far=1e4, stepsize=stepsize, bg=bg)
    poses = unbounded_cameras(n_train + n_test, gen)
    K = [[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]]
    rays = []
    for c2w in poses:
        o, d, v = camera_rays(H, W, focal, c2w)
        o, d, v = o.to(device), d.to(device), v.to(device)
        rgb = torch.cat([gt(o[i:i + 8192], d[i:i + 8192], v[i:i + 8192], **render_kwargs)['rgb_marched']
                         for i in range(0, o.shape[0], 8192)])
        rays.append((o, d, v, rgb))
    cat = lambda k: torch.cat([rays[i][k] for i in range(n_train)]).contiguous()     # noqa: E731
    return dict(gt=gt, rays_o=cat(0), rays_d=cat(1), viewdirs=cat(2), target=cat(3), render_kwargs=render_kwargs,
                test_poses=poses[n_train:].numpy(), test_HW=np.array([[H, W]] * n_test), test_Ks=np.array([K] * n_test, np.float32),
                test_images=[rays[n_train + i][3].reshape(H, W, 3).cpu().numpy() for i in range(n_test)],
                train_poses=poses[:n_train].numpy(), bg_len=bg_len, world=world, H=H, W=W, focal=focal)
