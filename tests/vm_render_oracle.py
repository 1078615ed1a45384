"""The ray-differentiable render of VMTriPlaneVoxGO / TensoRFVoxGO(raygrad=True) restated in float64 torch ops on the CPU, for
tools/vm_raygrad_descent_cpu.py (which chooses the capture of the recovery test) and the models of
tests/test_gpu_vm_raygrad.py.  Test infrastructure; the capture and the pose errors are tests/hash_render_oracle.py's.

The restatement is DirectVoxGO._forward_raygrad's op sequence: positions o + d * lam with lam a constant, the dense density by
F.grid_sample ('vm') or the sum of planes times lines ('tensorf': vm_oracle.torch_restatement, summed), Raw2Alpha, the two
fast_color_thres filters as fixed sets from a no-grad pass, the features vm_oracle.torch_restatement @ basis, the colour
head, the per-ray sum.  Without cells in the record (the descent) the cells are F.grid_sample's own, chosen in the dtype; with
`rec['cells']` (cells_of: the float32 run's cells, the weights alone from the positions) the restatement is the function the
kernels differentiate in either dtype, which is what tests/test_gpu_vm_raygrad.py bounds the device's ray gradients against."""
import copy

import numpy as np
import torch
import torch.nn.functional as F

import hash_render_oracle as RO
import vm_oracle as VO

KEYS = VO.KEYS


def _bumps(n, centre, width):
    t = torch.linspace(-1, 1, n)
    return torch.exp(-((t - centre) / width) ** 2)


def make_model(which, world, seed, raygrad=True, **kw):
    """R = 4.  'vm': a VMTriPlaneVoxGO with scenes.blob_density copied into its grid (tests/hash_render_oracle's
    construction).  'tensorf': a TensoRFVoxGO whose density is separable bumps (component 0 of every plane / line pair: a
    Gaussian in the plane times a Gaussian along the line, amplitude 9 each pair) plus a negative constant (component 1:
    plane 1, line -1, so -3 in all) and small noise in the other components; its occupancy mask is left all True."""
    from directvoxgo_amd import scenes
    from directvoxgo_amd.tensorf import TensoRFVoxGO
    from directvoxgo_amd.vm import VMTriPlaneVoxGO
    gen = torch.Generator().manual_seed(seed)
    mn, mx = torch.full((3,), -RO.HALF), torch.full((3,), RO.HALF)
    torch.manual_seed(seed)
    base = dict(num_voxels=world ** 3, num_voxels_base=world ** 3, alpha_init=1e-2, fast_color_thres=1e-4, n_comp=4,
                rgbnet_dim=6, rgbnet_width=64, raygrad=raygrad)
    if which == 'vm':
        m = VMTriPlaneVoxGO(mn, mx, **{**base, **kw})
        ws = tuple(int(v) for v in m.world_size)
        density = scenes.blob_density(ws, mn, mx, gen)
        alpha = torch.nn.functional.max_pool3d(scenes.activate(density, m.act_shift, 1.0)[None, None], 3, 1, 1)[0, 0]
        with torch.no_grad():
            m.density.copy_(density[None, None])
            m.mask_cache.mask.copy_(alpha > 1e-4)
    else:
        m = TensoRFVoxGO(mn, mx, density_n_comp=4, **{**base, **kw})
        with torch.no_grad():
            for i, k in enumerate(('xy', 'yz', 'zx')):
                p, ln = m.density_planes[k], m.density_lines[k]
                p.copy_(torch.randn(p.shape, generator=gen) * 0.05)
                ln.copy_(torch.randn(ln.shape, generator=gen) * 0.05)
                H, W, N = p.shape[2], p.shape[3], ln.shape[2]
                c = 0.25 * (i - 1)
                p[0, 0] = 3.0 * _bumps(H, c, 0.45)[:, None] * _bumps(W, -c, 0.45)[None, :]
                ln[0, 0, :, 0] = 3.0 * _bumps(N, 0.1 * i, 0.45)
                p[0, 1] = 1.0
                ln[0, 1] = -1.0
            m.mask_cache.mask.fill_(True)
    with torch.no_grad():
        for t in list(m.planes.values()) + list(m.lines.values()):
            t.copy_(torch.randn(t.shape, generator=gen) * 0.5)
        for p in m.rgbnet.parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * 0.1)
    return m


def _detached(params, dtype):
    return {k: params[k].detach().cpu().contiguous().to(dtype) for k in KEYS}


def raw_density(m, pts, dtype):
    mn, mx = m.xyz_min.detach().cpu().to(dtype), m.xyz_max.detach().cpu().to(dtype)
    if getattr(m, 'density', None) is not None:
        ind = ((pts - mn) / (mx - mn)).flip((-1,)) * 2 - 1
        return F.grid_sample(m.density.detach().cpu().to(dtype), ind.reshape(1, 1, 1, -1, 3), mode='bilinear', align_corners=True).reshape(-1)
    return VO.torch_restatement(_detached(m.density_planes, dtype), _detached(m.density_lines, dtype), pts, mn, mx).sum(-1)


def _alpha(m, dens, rk):
    shift = float(m.act_shift) + float(getattr(m, 'density_offset', 0.0))
    return 1 - torch.pow(1 + torch.exp(dens + shift), -float(rk['stepsize'] * m.voxel_size_ratio))


def cpu_record(m, o, d, rk, cells=False):
    """The constants of a render of the rays o, d (tensors on the CPU) without a device: the CPU oracle's sampler and
    occupancy lookup, lam as the model computes it, the two filters from a no-grad float64 pass and, with `cells`, the float32
    cells of the sampler's positions (cells_of)."""
    from oracle import oracle as O
    mn, mx = m.xyz_min.detach().cpu().numpy(), m.xyz_max.detach().cpu().numpy()
    stepdist = float(np.float32(rk['stepsize'] * float(m.voxel_size)))
    o32, d32 = o.detach().float().numpy(), d.detach().float().numpy()
    pts, out, ray_id, step_id, _, t_min, _ = O.sample_pts_on_rays(o32, d32, mn, mx, rk['near'], rk['far'], stepdist)
    keep = ~out
    pts, ray_id, step_id = pts[keep], ray_id[keep], step_id[keep]
    keep = O.maskcache_lookup(m.mask_cache.mask.detach().cpu().numpy(), pts, m.mask_cache.xyz2ijk_scale.detach().cpu().numpy(),
                              m.mask_cache.xyz2ijk_shift.detach().cpu().numpy())
    pts, ray_id, step_id = pts[keep], ray_id[keep], step_id[keep]
    rid = torch.from_numpy(ray_id)
    lam = torch.from_numpy(t_min)[rid] + (stepdist * torch.from_numpy(step_id).float()) / d.detach().float().norm(dim=-1)[rid]
    with torch.no_grad():
        dt = torch.float64
        p = o.detach().to(dt)[rid] + d.detach().to(dt)[rid] * lam.to(dt)[:, None]
        alpha = _alpha(m, raw_density(m, p, dt), rk)
        m1 = alpha > m.fast_color_thres
        a1, r1 = alpha[m1], rid[m1]
        w1 = RO._transmittance(1 - a1 + 1e-10, r1, o.shape[0])[0] * a1
    return dict(ray_id0=rid, lam=lam, m1=m1, m2=w1 > m.fast_color_thres, cells=cells_of(m, pts) if cells else None)


def restate(m, o, d, v, rec, dtype, rk, vm_positions=True):
    """-> rgb_marched [N,3] in `dtype`, differentiable in o and d (tensors of `dtype` on the CPU).  With `rec['cells']`
    (cells_of) every interpolation takes the float32 run's cell and only its weights from the positions in `dtype`: the
    function the kernels differentiate, fit for an error bound; without it the cells are F.grid_sample's own.
    `vm_positions=False` (fixed cells only) detaches the positions the VM tensors are read at -- the features' and, in
    TensoRFVoxGO, the density's: what is left is the share of the ray gradient that does not pass through csrc/vm_xyz.hip."""
    from directvoxgo_amd.voxel_model import _posenc
    N = o.shape[0]
    mn, mx = m.xyz_min.detach().cpu().to(dtype), m.xyz_max.detach().cpu().to(dtype)
    rid0 = rec['ray_id0']
    pts = o[rid0] + d[rid0] * rec['lam'].to(dtype)[:, None]
    cells = rec.get('cells')
    m1, m2 = rec['m1'], rec['m2']
    pvm = pts if vm_positions else pts.detach()
    if cells is None:
        dens = raw_density(m, pts, dtype)
    elif 'ijk0' in cells:
        dens = RO.trilinear(m.density.detach().cpu()[0].to(dtype), pts, cells['ijk0'], cells['inb'], mn, mx)[:, 0]
    else:
        dens = vm_fixed(_detached(m.density_planes, dtype), _detached(m.density_lines, dtype), pvm, cells['density'], mn, mx).sum(-1)
    alpha = _alpha(m, dens, rk)
    alpha1, rid1 = alpha[m1], rid0[m1]
    act = rec.get('act1', torch.ones_like(alpha1, dtype=torch.bool))
    T, last = RO._transmittance(torch.where(act, 1 - alpha1 + 1e-10, torch.ones_like(alpha1)), rid1, N)
    w2, rid2 = torch.where(act, T * alpha1, torch.zeros_like(alpha1))[m2], rid1[m2]
    if cells is None:
        feat = VO.torch_restatement(_detached(m.planes, dtype), _detached(m.lines, dtype), pts[m1][m2], mn, mx)
    else:
        sel = {k: tuple(x[m1][m2] for x in c) for k, c in cells['features'].items()}
        feat = vm_fixed(_detached(m.planes, dtype), _detached(m.lines, dtype), pvm[m1][m2], sel, mn, mx)
    feat = feat @ m.basis.detach().cpu().to(dtype)
    net = copy.deepcopy(m.rgbnet).cpu().to(dtype)
    for p in net.parameters():
        p.requires_grad_(False)
    emb = _posenc(v.detach().cpu().to(dtype), m.viewfreq.detach().cpu().to(dtype))[rid2]
    rgb = torch.sigmoid(net(torch.cat([feat[:, 3:], emb], -1)) + feat[:, :3])
    return torch.zeros(N, 3, dtype=dtype).index_add(0, rid2, w2[:, None] * rgb) + last[:, None] * rk['bg']


# ------------------------------------------------------------------------------------------ fixed float32 cells
def _vm_cells(planes, lines, pts, mn, mx):
    """{key: (h0, w0, n0)} int64 tensors: the float32 cell and node of every position (vm_raygrad_oracle.inputs32)"""
    import vm_raygrad_oracle as VR
    out = {}
    for k in KEYS:
        I = VR.inputs32(k, planes[k].shape[2], planes[k].shape[3], lines[k].shape[2], pts, mn, mx)
        out[k] = (torch.from_numpy(I.h0), torch.from_numpy(I.w0), torch.from_numpy(I.n0))
    return out


def cells_of(m, pts):
    """The float32 cells of the positions `pts` [M,3] (numpy float32): of the colour planes and lines and of the density (the
    lattice's, raygrad_oracle.inputs32, or the density planes' and lines')."""
    import raygrad_oracle as R
    mn, mx = m.xyz_min.detach().cpu().numpy(), m.xyz_max.detach().cpu().numpy()
    cells = dict(features=_vm_cells(m.planes, m.lines, pts, mn, mx))
    if getattr(m, 'density', None) is not None:
        I = R.inputs32(pts, mn, mx, tuple(int(x) for x in m.density.shape[2:]))
        cells.update(ijk0=torch.from_numpy(I.ijk0), inb=torch.from_numpy(I.inb))
    else:
        cells['density'] = _vm_cells(m.density_planes, m.density_lines, pts, mn, mx)
    return cells


def vm_fixed(planes, lines, pts, cells, mn, mx):
    """[M, 3R] in the tensors' dtype: plane value times line value with the cell (h0, w0) and the node n0 fixed (`cells`:
    {key: (h0, w0, n0)}) and the weights from g in that dtype; corners and nodes out of range dropped (zero padding)."""
    import triplane_oracle as TO
    out = []
    for k in KEYS:
        p, ln = planes[k][0], lines[k][0, :, :, 0]
        dt = p.dtype
        h0, w0, n0 = cells[k]
        ah, aw = TO.AXES[k]
        al = VO.LINE_AXIS[k]

        def weights(a, size, f):
            w1 = (pts[:, a] - mn[a]) / (mx[a] - mn[a]) * (size - 1) - f.to(dt)
            return (1 - w1, w1)
        H, W, N = p.shape[1], p.shape[2], ln.shape[1]
        wh, ww, wn = weights(ah, H, h0), weights(aw, W, w0), weights(al, N, n0)
        pv = torch.zeros(pts.shape[0], p.shape[0], dtype=dt)
        for i in range(2):
            for j in range(2):
                ih, iw = h0 + i, w0 + j
                ok = (ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)
                v = p[:, ih.clamp(0, H - 1), iw.clamp(0, W - 1)].t()
                pv = pv + torch.where(ok[:, None], (wh[i] * ww[j])[:, None] * v, torch.zeros_like(v))
        lv = torch.zeros_like(pv)
        for i in range(2):
            n = n0 + i
            ok = (n >= 0) & (n < N)
            v = ln[:, n.clamp(0, N - 1)].t()
            lv = lv + torch.where(ok[:, None], wn[i][:, None] * v, torch.zeros_like(v))
        out.append(pv * lv)
    return torch.cat(out, -1)
