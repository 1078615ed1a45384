"""The graph of HashVoxGO's ray-differentiable render (DirectVoxGO._forward_raygrad on a hash-grid model) restated in torch
ops on the CPU, in float32 or float64, with its stop-gradients: lam, the kept sets, the cells (density lattice and every hash
level) and viewdirs are constants.  Test infrastructure: tests/test_gpu_hash_raygrad.py compares the device's ray gradients
with it (the record of constants then comes from the device run) and tools/hash_raygrad_descent_cpu.py descends on it (the
record then comes from the CPU oracle's sampler and a no-grad pass of this restatement).  It also builds the small models
and the capture both use, so that the tool's run is the test's.
"""
import copy
import math

import numpy as np
import torch

import hash_raygrad_oracle as HR
import raygrad_oracle as R

HALF = 1.5 * 1.05
MODEL = dict(n_levels=4, n_feat=2, log2_hashmap_size=10, base_res=8, max_res=64, rgbnet_width=64)


def make_model(world, seed, raygrad=True, **kw):
    """A small HashVoxGO on the CPU: scenes.blob_density, its occupancy mask from the density, head weights N(0, 0.1) and a
    table N(0, 0.5) (the constructor's U(+-1e-4) table makes colour independent of position)."""
    from directvoxgo_amd import scenes
    from directvoxgo_amd.hashgrid import HashVoxGO
    gen = torch.Generator().manual_seed(seed)
    mn, mx = torch.full((3,), -HALF), torch.full((3,), HALF)
    torch.manual_seed(seed)
    m = HashVoxGO(mn, mx, num_voxels=world ** 3, num_voxels_base=world ** 3, alpha_init=1e-2, fast_color_thres=1e-4,
                  raygrad=raygrad, **{**MODEL, **kw})
    ws = tuple(int(v) for v in m.world_size)
    density = scenes.blob_density(ws, mn, mx, gen)
    alpha = torch.nn.functional.max_pool3d(scenes.activate(density, m.act_shift, 1.0)[None, None], 3, 1, 1)[0, 0]
    with torch.no_grad():
        m.density.copy_(density[None, None])
        m.hash_table.copy_(torch.randn(m.hash_table.shape, generator=gen) * 0.5)
        for p in m.rgbnet.parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * 0.1)
        m.mask_cache.mask.copy_(alpha > 1e-4)
    assert 0.02 < float(m.mask_cache.mask.float().mean()) < 0.98
    return m


def capture(n_views=6, hw=24, focal=30.0, radius=4.0, seed=7, rot_deg=2.0, shift=0.03):
    """tests/test_gpu_raygrad.py's capture: cameras on a sphere about the origin, each turned by `rot_deg` about a random axis
    and moved by `shift` * radius.  -> true [n,3,4], noisy [n,3,4], HW [n,2], Ks [n,3,3]"""
    from directvoxgo_amd import scenes
    from directvoxgo_amd.pose import se3_exp
    gen = torch.Generator().manual_seed(seed)
    true = torch.stack([scenes.pose_spherical(60.0 * i + 10.0, -30.0 - 5.0 * (i % 3), radius)[:3, :4] for i in range(n_views)])
    axis = torch.randn(n_views, 3, generator=gen)
    axis = axis / axis.norm(dim=-1, keepdim=True)
    move = torch.randn(n_views, 3, generator=gen)
    move = move / move.norm(dim=-1, keepdim=True) * (shift * radius)
    E = se3_exp(torch.cat([axis * math.radians(rot_deg), torch.zeros(n_views, 3)], -1))[:, :, :3]
    noisy = torch.cat([E @ true[:, :, :3], true[:, :, 3:] + move[:, :, None]], -1)
    K = np.array([[focal, 0, 0.5 * hw], [0, focal, 0.5 * hw], [0, 0, 1]], np.float32)
    return true, noisy, np.array([[hw, hw]] * n_views), np.stack([K] * n_views)


def pose_errors(est, true):
    """-> (rotation error [n] in radians, translation error [n])"""
    est, true = est.detach().cpu().double(), true.cpu().double()
    rel = est[:, :, :3] @ true[:, :, :3].transpose(1, 2)
    cos = ((rel.diagonal(dim1=1, dim2=2).sum(-1) - 1) / 2).clamp(-1, 1)
    return torch.acos(cos), (est[:, :, 3] - true[:, :, 3]).norm(dim=-1)


# ------------------------------------------------------------------------------------------ the constants of a render
def cells_of(m, pts):
    """The float32 cells of the positions `pts` [M,3] (numpy float32): the density lattice's (raygrad_oracle.inputs32) and every
    hash level's (hash_raygrad_oracle.inputs32), as tensors."""
    mn, mx = m.xyz_min.detach().cpu().numpy(), m.xyz_max.detach().cpu().numpy()
    ws = tuple(int(x) for x in m.density.shape[2:])
    I = R.inputs32(pts, mn, mx, ws)
    levels = []
    for l in range(m.levels.L):
        H = HR.inputs32(pts, mn, mx, m.levels.res, l)
        levels.append((torch.from_numpy(H.f), torch.from_numpy(H.inside), torch.from_numpy(H.w.astype(np.float64))))
    return dict(ijk0=torch.from_numpy(I.ijk0), inb=torch.from_numpy(I.inb), levels=levels)


def trilinear(grid, pts, ijk0, inb, mn, mx):
    """grid [C,X,Y,Z], the cell fixed (ijk0, inb from the float32 positions), the weights from g in grid's dtype; zero padding"""
    size = torch.tensor(grid.shape[1:], dtype=grid.dtype)
    g = (pts - mn) / (mx - mn) * (size - 1)
    w1 = g - ijk0.to(grid.dtype)
    w = torch.stack([1 - w1, w1], -1)                        # [M,3,2]
    out = torch.zeros(pts.shape[0], grid.shape[0], dtype=grid.dtype)
    for n in range(8):
        b = ((n >> 2) & 1, (n >> 1) & 1, n & 1)
        idx = [(ijk0[:, a] + b[a]).clamp(0, grid.shape[1 + a] - 1) for a in range(3)]
        v = grid[:, idx[0], idx[1], idx[2]].t()
        wn = (w[:, 2, b[2]] * w[:, 1, b[1]]) * w[:, 0, b[0]]
        out = out + torch.where(inb[:, n, None], wn[:, None] * v, torch.zeros_like(v))
    return out


def hash_features(table, pts, levels, mn, mx, res, offsets):
    """table [T,F] -> [M, L F] in the table's dtype: the cell of every level fixed (`levels`: cells_of(...)['levels']), the
    weights from g in that dtype where the position is inside on the axis and the float32 run's constants where the clamp acts."""
    import hash_oracle as HO
    out = []
    for l, (f, inside, wconst) in enumerate(levels):
        size = torch.tensor([int(v) for v in res[l]], dtype=table.dtype)
        g = (pts - mn) / (mx - mn) * (size - 1)
        w1 = torch.where(inside, g - f.to(table.dtype), wconst[:, :, 1].to(table.dtype))
        w = torch.stack([1 - w1, w1], -1)
        acc = torch.zeros(pts.shape[0], table.shape[1], dtype=table.dtype)
        for n in range(8):
            b = ((n >> 2) & 1, (n >> 1) & 1, n & 1)
            rows = int(offsets[l]) + HO.node_rows(res, offsets, l, *[(f[:, a] + b[a]).numpy() for a in range(3)])
            wn = (w[:, 0, b[0]] * w[:, 1, b[1]]) * w[:, 2, b[2]]
            acc = acc + wn[:, None] * table[torch.from_numpy(rows)]
        out.append(acc)
    return torch.cat(out, -1)


def _transmittance(f, ray_id, N):
    """f [M] per-sample factors of rays whose samples are consecutive -> (the exclusive running product per ray [M], the
    product of every ray [N]; 1 for a ray without samples): a cumprod per ray, as tests/test_gpu_raygrad.py restates it"""
    counts = torch.bincount(ray_id, minlength=N).tolist()
    T, last = [], []
    for seg in torch.split(f, counts):
        c = torch.cumprod(seg, 0)
        T.append(torch.cat([torch.ones(1, dtype=f.dtype), c[:-1]]) if len(seg) else seg)
        last.append(c[-1] if len(seg) else torch.ones((), dtype=f.dtype))
    return torch.cat(T), torch.stack(last)


def restate(m, o, d, v, rec, dtype, rk, feature_positions=True):
    """-> rgb_marched [N,3] in `dtype`, differentiable in o and d (tensors of `dtype` on the CPU).  `rec`: ray_id0, lam, m1,
    act1, m2 and the cells of the samples that passed the occupancy mask (cells_of).  `feature_positions=False` detaches the
    positions the hash features are read at: what is left is the density's share of the ray gradient."""
    from directvoxgo_amd.voxel_model import _posenc
    N = o.shape[0]
    mn, mx = m.xyz_min.detach().cpu().to(dtype), m.xyz_max.detach().cpu().to(dtype)
    rid0 = rec['ray_id0']
    pts = o[rid0] + d[rid0] * rec['lam'].to(dtype)[:, None]
    dens = trilinear(m.density.detach().cpu()[0].to(dtype), pts, rec['ijk0'], rec['inb'], mn, mx)[:, 0]
    interval = float(rk['stepsize'] * m.voxel_size_ratio)
    alpha = 1 - torch.pow(1 + torch.exp(dens + float(m.act_shift)), -interval)
    m1, m2, act = rec['m1'], rec['m2'], rec['act1']
    alpha1, rid1 = alpha[m1], rid0[m1]
    f = torch.where(act, 1 - alpha1 + 1e-10, torch.ones_like(alpha1))
    T, last = _transmittance(f, rid1, N)
    w1 = torch.where(act, T * alpha1, torch.zeros_like(alpha1))
    w2, rid2 = w1[m2], rid1[m2]
    sel = lambda x: x[m1][m2]                                       # noqa: E731
    p2 = sel(pts) if feature_positions else sel(pts).detach()
    feat = hash_features(m.hash_table.detach().cpu().to(dtype), p2, [tuple(sel(x) for x in lv) for lv in rec['levels']], mn, mx,
                         m.levels.res, m.levels.offsets)
    net = copy.deepcopy(m.rgbnet).cpu().to(dtype)
    for p in net.parameters():
        p.requires_grad_(False)
    emb = _posenc(v.detach().cpu().to(dtype), m.viewfreq.detach().cpu().to(dtype))[rid2]
    rgb = torch.sigmoid(net(torch.cat([feat[:, 3:], emb], -1)) + feat[:, :3])
    return torch.zeros(N, 3, dtype=dtype).index_add(0, rid2, w2[:, None] * rgb) + last[:, None] * rk['bg']


def cpu_record(m, o, d, rk):
    """The constants of a render of the rays o, d (float32 tensors on the CPU) without a device: the oracle's sampler and
    occupancy lookup, lam as the model computes it, the float32 cells, and the two filters from a no-grad float64 pass."""
    from oracle import oracle as O
    mn, mx = m.xyz_min.detach().cpu().numpy(), m.xyz_max.detach().cpu().numpy()
    stepdist = float(np.float32(rk['stepsize'] * float(m.voxel_size)))
    o32, d32 = o.detach().float().numpy(), d.detach().float().numpy()
    pts, out, ray_id, step_id, _, t_min, _ = O.sample_pts_on_rays(o32, d32, mn, mx, rk['near'], rk['far'], stepdist)
    keep = ~out
    pts, ray_id, step_id = pts[keep], ray_id[keep], step_id[keep]
    mask = m.mask_cache.mask.detach().cpu().numpy()
    scale = m.mask_cache.xyz2ijk_scale.detach().cpu().numpy()
    shift = m.mask_cache.xyz2ijk_shift.detach().cpu().numpy()
    keep = O.maskcache_lookup(mask, pts, scale, shift)
    pts, ray_id, step_id = pts[keep], ray_id[keep], step_id[keep]
    rid = torch.from_numpy(ray_id)
    lam = torch.from_numpy(t_min)[rid] + (stepdist * torch.from_numpy(step_id).float()) / d.detach().float().norm(dim=-1)[rid]
    rec = dict(ray_id0=rid, lam=lam, **cells_of(m, pts))
    with torch.no_grad():                                           # the two fast_color_thres filters
        dt = torch.float64
        p = o.detach().to(dt)[rid] + d.detach().to(dt)[rid] * lam.to(dt)[:, None]
        dens = trilinear(m.density.detach().cpu()[0].to(dt), p, rec['ijk0'], rec['inb'], m.xyz_min.detach().cpu().to(dt),
                         m.xyz_max.detach().cpu().to(dt))[:, 0]
        alpha = 1 - torch.pow(1 + torch.exp(dens + float(m.act_shift)), -float(rk['stepsize'] * m.voxel_size_ratio))
        m1 = alpha > m.fast_color_thres
        a1, r1 = alpha[m1], rid[m1]
        w1 = _transmittance(1 - a1 + 1e-10, r1, o.shape[0])[0] * a1
        rec.update(m1=m1, act1=torch.ones_like(a1, dtype=torch.bool), m2=w1 > m.fast_color_thres)
    return rec
