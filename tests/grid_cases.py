"""The inputs of tests/test_gpu_grid_oracle.py, by name, and what each is there for.  CPU only; tests/test_grid_oracle_host.py
asserts, before anything is launched from them, that the float32 setup lands where every row says.

Box: xyz_min = (-0.5, -1.25, -0.25), xyz_max = (1.5, 2.75, 0.75) -- not cubic, not centred; the extents are powers of two,
so that lattice nodes can be hit exactly.  A point is built from its voxel coordinate g and mapped back to the world:
p = min + g / (size - 1) * (max - min), rounded to float32; where g is an integer the neighbouring float32 values are
searched for the one whose restated setup gives g exactly (weights 1 and 0), and the row is dropped if there is none.

Edge rows of a lattice (`edge_rows`), each a list of points:
    nodes         exactly on lattice nodes on all axes / on one axis, the others fractional: weights 1 and 0
    faces         g = 0 and g = size - 1 on one axis (the upper corner of the upper face is out of range, weight 0)
    out1/2/3      g in (-1, 0) or (size - 1, size) on one, two, three axes: only some corners are in range
    beyond        g < -1 or g > size on one axis: no corner in range
    corners       the eight corners of the box
    pile_inside   4096 coincident points in one interior cell        } chains of 4096 atomic additions
    pile_face     4096 coincident points on the upper face of an axis }
Random rows (`random_points`): M in {1, 255, 256, 257, 5003} points, a third of them outside on some axis; M and M * C
cross the 256-thread block edge for C in {3, 9, 12}.

Rows that cannot be built:
    non-finite coordinates       brick_oracle.tri_setup refuses them, and (int)NaN is not defined in the kernel either
    out / beyond on a unit axis  size == 1 gives g = ((c + 1) / 2) * 0 = 0 for every finite p: floor corner 0, upper
                                 corner out of range, whatever the position.  Such an axis is kept at g = 0 in every row
                                 and the out1/2/3 and beyond entries that would move along it are left out.
    interior nodes of (2, 2, 2)  every node is a box corner (row 'corners').
"""
import numpy as np

import brick_oracle as B

MN = np.array([-0.5, -1.25, -0.25], np.float32)
MX = np.array([1.5, 2.75, 0.75], np.float32)
LATTICES = [(2, 2, 2), (5, 7, 9), (17, 4, 33), (1, 5, 6), (5, 1, 6), (5, 6, 1)]
CHANNELS = [1, 3, 4, 9, 12]
SAMPLE_COUNTS = [1, 255, 256, 257, 5003]
PILE = 4096
_FRAC = (0.3, 0.55, 0.7)
_UNIT_AT = 0.37                                   # where in the box a point sits along a unit axis


def inner(dims):
    """a fractional voxel coordinate in an interior cell (unit axes: 0)"""
    return np.array([0.0 if s == 1 else min(s - 2, (s - 1) // 2) + f for s, f in zip(dims, _FRAC)])


def _plain(g, dims):
    size1 = np.array(dims, np.float64) - 1
    ext = MX.astype(np.float64) - MN
    with np.errstate(all='ignore'):
        p = np.where(size1 > 0, MN + np.asarray(g, np.float64) / np.where(size1 > 0, size1, 1) * ext, MN + _UNIT_AT * ext)
    return p.astype(np.float32)


_node_cache = {}


def _node(a, k, dims):
    """float32 coordinate on axis a whose restated setup gives g == k exactly, or None"""
    key = (a, k, dims)
    if key not in _node_cache:
        base = _plain(inner(dims), dims)
        c0 = _plain(np.where(np.arange(3) == a, k, inner(dims)), dims)[a]
        cands = [c0]
        up = dn = c0
        for _ in range(8):
            up, dn = np.nextafter(up, np.float32(np.inf)), np.nextafter(dn, np.float32(-np.inf))
            cands += [up, dn]
        pts = np.repeat(base[None], len(cands), 0)
        pts[:, a] = cands
        ijk0, w, _, _ = B.tri_setup(pts, MN, MX, *dims)
        q = 4 >> a                                           # the corner that differs from corner 0 on axis a only
        ok = (ijk0[:, a] == k) & (w[:, q] == 0) & (w[:, 0] > 0)
        _node_cache[key] = np.float32(cands[int(np.argmax(ok))]) if ok.any() else None
    return _node_cache[key]


def points(g, dims):
    """g [n, 3] voxel coordinates -> (xyz [n, 3] float32, i0 [n, 3] the floor corners the row claims)"""
    g = np.asarray(g, np.float64).reshape(-1, 3)
    xyz = _plain(g, dims)
    for a, s in enumerate(dims):
        if s == 1:
            continue
        for k in np.unique(g[g[:, a] == np.round(g[:, a]), a]):
            p = _node(a, int(k), dims)
            assert p is not None, f'no float32 coordinate lands on node {int(k)} of axis {a} of {dims}'
            xyz[g[:, a] == k, a] = p
    i0 = np.where(np.array(dims) == 1, 0, np.floor(g)).astype(np.int64)
    return xyz, i0


def in_range(i0, dims):
    """[n, 8] bool: the corners of floor corner i0 that lie in the lattice (corner bit 2 = +X, 1 = +Y, 0 = +Z)"""
    out = np.ones((i0.shape[0], 8), bool)
    for q in range(8):
        for a, s in enumerate(dims):
            i = i0[:, a] + ((q >> (2 - a)) & 1)
            out[:, q] &= (i >= 0) & (i < s)
    return out


def node_index(a, dims):
    """an interior node of axis a that float32 can hit exactly (else the lower face)"""
    for k in range(1, dims[a] - 1):
        if _node(a, k, dims) is not None:
            return k
    return 0


def edge_rows(dims):
    """-> [(name, g [n, 3])]"""
    s = np.array(dims)
    free = [a for a in range(3) if dims[a] > 1]
    mid = inner(dims)
    lo_out, hi_out = -0.4, s - 1 + 0.6
    rows = []
    nodes = [np.array([node_index(a, dims) if dims[a] > 1 else 0 for a in range(3)], float)]
    for a in free:
        g = mid.copy(); g[a] = node_index(a, dims); nodes.append(g)
    rows.append(('nodes', np.stack(nodes)))
    faces = []
    for a in free:
        for v in (0, s[a] - 1):
            g = mid.copy(); g[a] = v; faces.append(g)
    rows.append(('faces', np.stack(faces)))
    for count in (1, 2, 3):
        out = []
        for mask in range(1, 8):
            axes = [a for a in range(3) if (mask >> a) & 1]
            if len(axes) != count or any(dims[a] == 1 for a in axes):
                continue
            for sides in range(1 << count):
                g = mid.copy()
                for j, a in enumerate(axes):
                    g[a] = hi_out[a] if (sides >> j) & 1 else lo_out
                out.append(g)
        if out:
            rows.append((f'out{count}', np.stack(out)))
    beyond = []
    for a in free:
        for v in (-1.7, s[a] + 0.8):
            g = mid.copy(); g[a] = v; beyond.append(g)
    rows.append(('beyond', np.stack(beyond)))
    rows.append(('corners', np.array([[(s[a] - 1) * ((i >> a) & 1) for a in range(3)] for i in range(8)], float)))
    rows.append(('pile_inside', np.repeat(mid[None], PILE, 0)))
    g = mid.copy(); g[free[0]] = s[free[0]] - 1
    rows.append(('pile_face', np.repeat(g[None], PILE, 0)))
    return rows


def edge_points(dims):
    """all edge rows of a lattice as one point list"""
    return np.concatenate([points(g, dims)[0] for _, g in edge_rows(dims)])


def random_points(dims, M, seed):
    rng = np.random.default_rng(seed)
    s = np.array(dims, float)
    g = rng.uniform(0, 1, (M, 3)) * (s - 1)
    out = rng.uniform(size=(M, 3)) < 0.12
    g = np.where(out, rng.uniform(-1.3, s + 0.3, (M, 3)), g)
    return _plain(g, dims)


def grad_out(M, C, seed):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((M, C)).astype(np.float32)
    g[::7, 0] = 0
    return g


def grid_values(C, dims, seed):
    return np.random.default_rng(seed).standard_normal((C, *dims)).astype(np.float32)


# ------------------------------------------------------------------------------------------ view weights
VIEW_DIMS = (9, 7, 11)
VIEW_NEAR, VIEW_FAR = 0.2, 9.0
VIEW_SAMPLES = [1, 63, 64, 65, 200]
VIEW_RAYS = [1, 5, 256]


def voxel_len(dims):
    return float(((MX - MN) / (np.array(dims, np.float32) - 1)).min())


def view_rays(n_rays, seed):
    """camera-like rays towards the box; the first five are the special ones (as many as fit): a zero direction
    component on two axes, on one axis, a ray that misses the box, a ray that starts inside, a ray pointing away"""
    rng = np.random.default_rng(seed)
    ctr, half = 0.5 * (MX + MN), 0.5 * (MX - MN)
    o = rng.standard_normal((n_rays, 3))
    o = ctr + o / np.linalg.norm(o, axis=1, keepdims=True) * rng.uniform(3.0, 4.5, (n_rays, 1))
    tgt = ctr + rng.uniform(-0.9, 0.9, (n_rays, 3)) * half
    d = (tgt - o) * rng.uniform(0.3, 1.5, (n_rays, 1))
    o, d = o.astype(np.float32), d.astype(np.float32)
    special = [([-3.0, 0.2, 0.1], [1.5, 0, 0]), ([0.3, -4.0, 0.2], [0.1, 2.0, 0]), ([4, 5, 3], [1, 0.1, 0.1]),
               ([0.4, 0.6, 0.3], [0.3, 0.5, -0.2]), ([0.2, 0.1, 5], [0, 0, 1])]
    for i, (so, sd) in enumerate(special[:n_rays]):
        o[i], d[i] = so, sd
    return o, d


def view_case(n_rays, n_samples):
    """-> dict(rays_o, rays_d, near, far, step, n_samples, dims): 0.37 voxel per step, so neighbours share voxels"""
    o, d = view_rays(n_rays, 100 * n_rays + n_samples)
    return dict(rays_o=o, rays_d=d, near=VIEW_NEAR, far=VIEW_FAR, step=np.float32(0.37 * voxel_len(VIEW_DIMS)), n_samples=n_samples,
                dims=VIEW_DIMS)


LINE_DIMS = (17, 5, 9)                            # voxel length 1/8, 1, 1/8: every node and every sample position is exact


def line_case(n_rays=5, n_samples=200):
    """n_rays copies of one ray along the lattice line (j, k) = (2, 3), one voxel per step, starting one unit before the
    box: t_min = 1, positions min_x + k / 8 exactly, every sum an exact integer (n_rays on the 17 voxels of the line)."""
    o = np.array([[MN[0] - 1.0, MN[1] + 2.0, MN[2] + 3 / 8.0]] * n_rays, np.float32)
    d = np.array([[1.0, 0.0, 0.0]] * n_rays, np.float32)
    return dict(rays_o=o, rays_d=d, near=0.5, far=9.0, step=np.float32(0.125), n_samples=n_samples, dims=LINE_DIMS)


def contended_case():
    """(2, 2, 2) lattice, 200 samples per ray inside one cell: eight keys for the whole wave"""
    o, d = view_rays(5, 7)
    return dict(rays_o=o, rays_d=d, near=VIEW_NEAR, far=VIEW_FAR, step=np.float32(0.004), n_samples=200, dims=(2, 2, 2))


OVERFLOW_DIMS = (220, 2, 3)
# found by `search_overflow`; tests/test_grid_oracle_host.py re-derives the certificate of exactly this input
OVERFLOW_CHOICE = dict(x0=0.25, j0=0, k0=0, stride=3.43)


def overflow_case(x0=OVERFLOW_CHOICE['x0'], j0=OVERFLOW_CHOICE['j0'], k0=OVERFLOW_CHOICE['k0'], stride=OVERFLOW_CHOICE['stride'],
                  n_rays=3, dims=OVERFLOW_DIMS):
    """Rays along x through the cell row (j0, k0) of a long thin lattice, `stride` voxels per step, 64 samples: every
    sample has eight keys of its own, the chunk 512.  The rays start inside the box, half a unit before the first sample
    (t_min is clamped to near = 0.5), which sits at the voxel coordinate x0.

    The table's multiplicative hash spreads keys of one constant stride almost evenly (a golden-ratio sequence), so an
    integer stride on a (132, 4, 4) lattice fills the table without a provable overflow: `search_overflow` finds no
    certificate there for strides 2.00 .. 2.05, the most that lattice has room for.  A fractional stride on a thinner
    lattice (keys (2 i + j) 3 + k, i advancing by 3 or 4) clusters: of the 512 keys of the chosen input, 238 have their
    whole probe window inside a range of 191 slots, so at least 47 of them take the fall-back to the global atomic in
    every insertion order.  220 x 2 x 3 = 1320 voxels."""
    ext = (MX - MN).astype(np.float64)
    vx = ext[0] / (dims[0] - 1)
    y = MN[1] + (j0 + 0.45) / (dims[1] - 1) * ext[1]
    z = MN[2] + (k0 + 0.6) / (dims[2] - 1) * ext[2]
    o = np.array([[MN[0] + x0 * vx - 0.5, y, z]] * n_rays, np.float32)
    d = np.array([[1.0, 0.0, 0.0]] * n_rays, np.float32)
    return dict(rays_o=o, rays_d=d, near=0.5, far=9.0, step=np.float32(stride * vx), n_samples=64, dims=dims)


def overflow_keys(**kw):
    """the keys one ray of `overflow_case` inserts in its only chunk"""
    import grid_oracle as G
    c = overflow_case(n_rays=1, **kw)
    pos = G.view_positions(c['rays_o'], c['rays_d'], MN, MX, c['near'], c['far'], c['step'], c['n_samples'])
    return G.chunk_keys(pos[0], MN, MX, c['dims'], 0)


def search_overflow(dims, strides):
    """Every (j0, k0, stride) on `dims` whose chunk has 512 distinct keys and provably overflows -> [(kwargs, certificate)]"""
    import grid_oracle as G
    found = []
    for stride in strides:
        for j0 in range(dims[1] - 1):
            for k0 in range(dims[2] - 1):
                kw = dict(x0=0.25, j0=j0, k0=k0, stride=float(stride), dims=dims)
                keys = overflow_keys(**kw)
                cert = G.overflow_certificate(keys) if np.unique(keys).size == 512 else None
                if cert is not None:
                    found.append((kw, cert))
    return found


# ------------------------------------------------------------------------------------------ the view count
COUNT_DIMS = (17, 19, 23)
COUNT_MIN, COUNT_MAX = np.array([-0.9, -0.8, -1.3], np.float32), np.array([0.8, 1.1, 1.0], np.float32)
COUNT_VOXELS = int(17 * 19 * 23 * 1.03)           # (extent / voxel_size).long() == (17, 19, 23) with room on both sides
COUNT_STEPSIZE, COUNT_NEAR, COUNT_FAR, COUNT_VIEWS, COUNT_SIDE = 0.5, 0.2, 6.0, 3, 24


def count_case():
    """3 views of 24 x 24 camera-like rays.  -> dict(rays_o, rays_d [3, 24, 24, 3], voxel_size, step, n_samples)"""
    import torch
    ext = torch.from_numpy(COUNT_MAX) - torch.from_numpy(COUNT_MIN)
    voxel_size = (ext.prod() / COUNT_VOXELS).pow(1 / 3)                 # DirectVoxGO._set_grid_resolution, same operations
    assert tuple((ext / voxel_size).long().tolist()) == COUNT_DIMS
    rng = np.random.default_rng(11)
    ctr, half = 0.5 * (COUNT_MAX + COUNT_MIN), 0.5 * (COUNT_MAX - COUNT_MIN)
    n = COUNT_SIDE * COUNT_SIDE
    ros, rds = [], []
    for v in range(COUNT_VIEWS):
        cam = rng.standard_normal(3)
        cam = ctr + cam / np.linalg.norm(cam) * 3.0
        tgt = ctr + rng.uniform(-1.0, 1.0, (n, 3)) * half
        d = tgt - cam
        d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.8, 1.2, (n, 1))
        ros.append(np.repeat(cam[None], n, 0)); rds.append(d)
    shape = (COUNT_VIEWS, COUNT_SIDE, COUNT_SIDE, 3)
    n_samples = int(np.linalg.norm(np.array(COUNT_DIMS) + 1) / COUNT_STEPSIZE) + 1
    step = float(np.float32(COUNT_STEPSIZE) * voxel_size.numpy().astype(np.float32))
    return dict(rays_o=np.stack(ros).astype(np.float32).reshape(shape), rays_d=np.stack(rds).astype(np.float32).reshape(shape),
                voxel_size=float(voxel_size), step=step, n_samples=n_samples)


# ------------------------------------------------------------------------------------------ segment sum
SEG_HEAD = [0, 64, 1, 63, 65, 63, 0, 256, 257, 1, 62, 5003]
#  rows:       0   64 65 128 193 256    512  769 770 832
#  the segments end on lane 63 (rows 63, 127), on a wave edge (832 = 13 * 64), on a block edge (256, 512); segment 0, 6 and
#  the last two are empty; lengths 1, 63, 64, 65, 256, 257 and 5003 all occur


def segment_case(C, seed=0):
    """-> dict(src [M, C], index [M], out0 [N, C]) ; C == 1 keeps the trailing axis (the caller squeezes for the 1-D form)"""
    rng = np.random.default_rng(40 + seed + C)
    lens = SEG_HEAD + [int(v) for v in rng.integers(1, 100, 20)] + [3, 0, 0]
    if sum(lens) % 64 == 0:
        lens[-3] += 1
    lens = np.array(lens)
    N, M = lens.shape[0], int(lens.sum())
    index = np.repeat(np.arange(N), lens)
    src = (rng.standard_normal((M, C)) * 10.0 ** rng.uniform(-3, 3, (M, 1))).astype(np.float32)
    # segments 3 and 8: large values in cancelling pairs plus small ones, so that mag >> |ref|
    for sgm in (3, 8):
        r = np.nonzero(index == sgm)[0]
        h = r.shape[0] // 2
        big = (rng.standard_normal((h, C)) * 1e4).astype(np.float32)
        src[r[:h]], src[r[h:2 * h]] = big, -big
        src[r[2 * h:]] = 1e-3
    out0 = rng.standard_normal((N, C)).astype(np.float32)
    return dict(src=src, index=index.astype(np.int64), out0=out0, lens=lens)
