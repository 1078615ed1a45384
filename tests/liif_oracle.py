"""Oracle of the LIIF plane decoder's kernels (csrc/liif.hip; lib/tri_dvgo.py:481-565 liif_interpolate), numpy.

Indices, MLP input rows and blend weights in float32, operation for operation what include/dvgo_hip.h states (the kernels
must give the same bits); the blend and the scatter in float64, with the sums of their absolute terms A and, for the
scatter, the number n of contributions per texel.

    plane   u (rows)   v (columns)   (Ta, Tb)
    xy      n_z        n_y           (Wx, Wy)
    yz      n_y        n_x           (Wy, Wz)
    zx      n_x        n_z           (Wz, Wx)

`decode` strings rows -> MLPs -> blend together in torch float64 on the oracle's indices and weights (differentiable in
the planes and the MLPs): what the reference fixture tests/golden/liif.npz is compared with.
"""
import numpy as np

KEYS = ('xy', 'yz', 'zx')
# world axis of u, of v; index into world_size of Ta, of Tb
TABLE = {'xy': (2, 1, 0, 1), 'yz': (1, 0, 1, 2), 'zx': (0, 2, 2, 0)}
NET_OF = {'xy': 'xy', 'yz': 'yz', 'zx': 'yz'}          # the reference's self.interp['zx'] = self.interp_yz
SHIFTS = ((-1, -1), (-1, 1), (1, -1), (1, 1))
U = 2.0 ** -24
f32 = np.float32
LO, HI = f32(-1 + 1e-6), f32(1 - 1e-6)


def _norm(p, mn, mx):
    return ((p.astype(f32) - f32(mn)) / (f32(mx) - f32(mn))) * f32(2) - f32(1)


def near(c, S):
    """grid_sample(mode='nearest', align_corners=False): rint (half to even) of the unnormalised coordinate, clipped."""
    r = np.rint(((c + f32(1)) * f32(S) - f32(1)) / f32(2))
    assert r.dtype == f32
    return np.clip(r, f32(0), f32(S - 1)).astype(np.int64)


def node(i, T):
    step = f32(2) / f32(T - 1) if T > 1 else f32(0)
    return i.astype(f32) * step - f32(1)


def geometry(key, H, W, xyz, mn, mx, world_size, local_ensemble=True):
    """-> row, col [E, M] int64; rel0, rel1, wgt [E, M] float32; (cell0, cell1) float32."""
    xyz = np.asarray(xyz, f32)
    au, av, ia, ib = TABLE[key]
    Ta, Tb = int(world_size[ia]), int(world_size[ib])
    u, v = _norm(xyz[:, au], mn[au], mx[au]), _norm(xyz[:, av], mn[av], mx[av])
    ra, rb = f32(1) / f32(Ta), f32(1) / f32(Tb)
    shifts = SHIFTS if local_ensemble else ((0, 0),)
    eps = f32(1e-6) if local_ensemble else f32(0)
    row, col, rel0, rel1, area = [], [], [], [], []
    for vx, vy in shifts:
        uc = np.minimum(np.maximum(u + (f32(vx) * ra + eps), LO), HI)
        vc = np.minimum(np.maximum(v + (f32(vy) * rb + eps), LO), HI)
        assert uc.dtype == f32 and vc.dtype == f32
        row.append(near(uc, H)); col.append(near(vc, W))
        q0, q1 = node(near(vc, Tb), Tb), node(near(uc, Ta), Ta)
        r0, r1 = (u - q0) * f32(H), (v - q1) * f32(W)
        rel0.append(r0); rel1.append(r1)
        area.append(np.abs(r0 * r1) + f32(1e-9))
    tot = area[0]
    for a in area[1:]:
        tot = tot + a
    wgt = np.stack([a / tot for a in area[::-1]])
    assert wgt.dtype == f32 and rel0[0].dtype == f32
    return np.stack(row), np.stack(col), np.stack(rel0), np.stack(rel1), wgt, (ra * f32(H), rb * f32(W))


def _chw(p):
    p = np.asarray(p)
    return p[0] if p.ndim == 4 else p


def rows(planes, xyz, mn, mx, world_size, cell_decode=True, local_ensemble=True):
    """-> inp [3, E, M, D] float32, wgt [3, E, M] float32: what dvgo_liif_gather writes, bit for bit."""
    inps, wgts = [], []
    for key in KEYS:
        p = _chw(planes[key]).astype(f32)
        C, H, W = p.shape
        row, col, rel0, rel1, wgt, (c0, c1) = geometry(key, H, W, xyz, mn, mx, world_size, local_ensemble)
        E, M = row.shape
        parts = [p[:, row, col].transpose(1, 2, 0), rel0[..., None], rel1[..., None]]
        if cell_decode:
            parts += [np.full((E, M, 1), c0, f32), np.full((E, M, 1), c1, f32)]
        inps.append(np.concatenate(parts, -1)); wgts.append(wgt)
    return np.stack(inps), np.stack(wgts)


def blend(pred, wgt, aggregation='concat'):
    """pred [3, E, M, C], wgt [3, E, M] -> (value, A) float64: [M, 3C] or [M, C]."""
    term = np.asarray(pred, np.float64) * np.asarray(wgt, np.float64)[..., None]
    v, a = term.sum(1), np.abs(term).sum(1)                  # over the shifts
    if aggregation == 'concat':
        return np.concatenate(list(v), 1), np.concatenate(list(a), 1)
    return (v[0] + v[1]) + v[2], (a[0] + a[1]) + a[2]


def scatter(shapes, xyz, mn, mx, world_size, grad_inp, local_ensemble=True):
    """shapes: {'xy': (C, H, W), ...}; grad_inp [3, E, M, D] -> {key: (grad [C, H, W], A [C, H, W], n [H, W])}."""
    g_all = np.asarray(grad_inp, np.float64)
    out = {}
    for s, key in enumerate(KEYS):
        C, H, W = shapes[key]
        row, col = geometry(key, H, W, xyz, mn, mx, world_size, local_ensemble)[:2]
        flat = (row * W + col).reshape(-1)
        g = g_all[s, :, :, :C].reshape(-1, C)
        grad = np.zeros((H * W, C)); A = np.zeros((H * W, C)); cnt = np.zeros(H * W, np.int64)
        np.add.at(grad, flat, g); np.add.at(A, flat, np.abs(g)); np.add.at(cnt, flat, 1)
        out[key] = (grad.reshape(H, W, C).transpose(2, 0, 1), A.reshape(H, W, C).transpose(2, 0, 1), cnt.reshape(H, W))
    return out


def decode(planes, nets, xyz, mn, mx, world_size, cell_decode=True, local_ensemble=True, aggregation='concat'):
    """torch, float64: planes {'xy', ...} of [1, C, H, W] tensors, nets {'xy', 'yz'} of float64 modules -> [M, 3C] or [M, C].
    Indices, relative coordinates, cells and weights are the float32 oracle's."""
    import torch
    outs = []
    for key in KEYS:
        p = planes[key]
        _, C, H, W = p.shape
        row, col, rel0, rel1, wgt, (c0, c1) = geometry(key, H, W, xyz, mn, mx, world_size, local_ensemble)
        E, M = row.shape
        feat = p[0][:, torch.from_numpy(row), torch.from_numpy(col)].permute(1, 2, 0).double()
        tail = [rel0[..., None], rel1[..., None]] + ([np.full((E, M, 1), c0), np.full((E, M, 1), c1)] if cell_decode else [])
        inp = torch.cat([feat, torch.from_numpy(np.concatenate(tail, -1).astype(np.float64))], -1)
        pred = nets[NET_OF[key]](inp.reshape(E * M, -1)).reshape(E, M, C)
        outs.append((pred * torch.from_numpy(wgt.astype(np.float64))[..., None]).sum(0))
    return torch.cat(outs, 1) if aggregation == 'concat' else (outs[0] + outs[1]) + outs[2]
