"""CPU statement of the mesh extraction, vectorised numpy, test infrastructure.

Written from the definition, not from csrc/mesh.hip: the tetrahedron cases are derived here geometrically (crossing-edge
midpoints, ordered around the inside-to-outside direction), where the kernel decides them with integer determinants.

  lattice_field(...)        the padded field of an extraction lattice (copy or trilinear, mask, padding)
  marching_tets(F, iso, mn, h) -> verts [V,3] f32, faces [F,3] int32, normals [V,3] f32

Definitions (shared with the kernel through the spec only):
  padded lattice P = R + 2, points in linear order (i * Py + j) * Pz + k; inside = F > iso (strict);
  directions d = x, y, z, xy, xz, yz, xyz; vertex id = vbase[p] + popcount(mask[p] & ((1 << d) - 1));
  cell p -> 6 tetrahedra {p, p + e_a, p + e_a + e_b, p + 1} for (a, b) in the permutation order xyz, xzy, yxz, yzx, zxy, zyx;
  faces in (cell, tetrahedron, triangle) order, right-hand normal from inside to outside; a quad (q0..q3) is cut along the
  diagonal through its smallest id: (q0,q1,q2),(q0,q2,q3) if min(q0,q2) < min(q1,q3), else (q0,q1,q3),(q1,q2,q3);
  vertex = mn + (i + t * e) * h with t = (iso - f0) / (f1 - f0), i the unpadded index of the edge's lower point;
  normal = -g / |g|, g = g0 + t (g1 - g0), g the clamped central difference of F over h per axis.
"""
import itertools

import numpy as np

DIRS = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)], np.int64)
PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
f32 = np.float32


def _dir_index(v):
    return int(np.nonzero((DIRS == np.asarray(v)).all(1))[0][0])


def tet_corners(perm):
    """corner offsets of one tetrahedron of the unit cell, ordered by inclusion"""
    e = np.eye(3, dtype=np.int64)
    c1 = e[perm[0]]
    c2 = c1 + e[perm[1]]
    return [np.zeros(3, np.int64), c1, c2, np.ones(3, np.int64)]


def _case_polygons(corners, inside):
    """the surface polygon of one tetrahedron case: a list of edges (lower corner offset, direction), ordered so that the
    right-hand normal points from the inside corners to the outside ones; [] when the case has no surface"""
    ins = [k for k in range(4) if inside[k]]
    out = [k for k in range(4) if not inside[k]]
    if not ins or not out:
        return []
    edges = [(a, b) for a in ins for b in out]
    mid = np.array([(corners[a] + corners[b]) / 2.0 for a, b in edges])
    n = np.mean([corners[k] for k in out], 0) - np.mean([corners[k] for k in ins], 0)
    c = mid.mean(0)
    u = mid[0] - c
    v = np.cross(n, u)
    ang = np.arctan2((mid - c) @ v, (mid - c) @ u)
    order = np.argsort(ang)                       # counter-clockwise seen from the tip of n
    poly = []
    for j in order:
        a, b = edges[j]
        lo, hi = (a, b) if a < b else (b, a)      # corners are ordered by inclusion: the lower index is the lower point
        poly.append((tuple(corners[lo]), _dir_index(corners[hi] - corners[lo])))
    return poly


def case_table():
    """{(tet, 4-bit inside mask over its corners): polygon}"""
    tab = {}
    for t, perm in enumerate(PERMS):
        cs = tet_corners(perm)
        for m in range(16):
            tab[(t, m)] = _case_polygons(cs, [(m >> k) & 1 for k in range(4)])
    return tab


def pad_field(values, iso, occupied=None):
    """[Rx,Ry,Rz] values -> [Rx+2,Ry+2,Rz+2] f32 with iso - 1 on the padding and where `occupied` is False"""
    empty = f32(iso) - f32(1)
    v = np.asarray(values, f32)
    if occupied is not None:
        v = np.where(occupied, v, empty).astype(f32)
    F = np.full(tuple(s + 2 for s in v.shape), empty, f32)
    F[1:-1, 1:-1, 1:-1] = v
    return F


def _fma32(a, b, c):
    """fp32 fma through float64 (the product of two floats is exact in double)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def trilinear(grid, gx, gy, gz):
    """grid [X,Y,Z] at continuous grid-index coordinates, the corner weights and corner order of grid_sample_fwd
    (zero outside the grid)"""
    X, Y, Z = grid.shape
    fx, fy, fz = np.floor(gx), np.floor(gy), np.floor(gz)
    i0, j0, k0 = fx.astype(np.int64), fy.astype(np.int64), fz.astype(np.int64)
    wx = ((fx + f32(1)) - gx, gx - fx)
    wy = ((fy + f32(1)) - gy, gy - fy)
    wz = ((fz + f32(1)) - gz, gz - fz)
    d = np.zeros(gx.shape, f32)
    for n in range(8):
        dx, dy, dz = (n >> 2) & 1, (n >> 1) & 1, n & 1
        i, j, k = i0 + dx, j0 + dy, k0 + dz
        ok = (i >= 0) & (i < X) & (j >= 0) & (j < Y) & (k >= 0) & (k < Z)
        v = grid[np.clip(i, 0, X - 1), np.clip(j, 0, Y - 1), np.clip(k, 0, Z - 1)]
        w = ((wz[dz] * wy[dy]) * wx[dx]).astype(f32)
        d = np.where(ok, _fma32(v, w, d), d)
    return d


def lattice_field(density, R, a, s, mn, h, iso, mask=None, mask_scale=None, mask_shift=None, copy=False):
    """The padded field of dvgo_mesh_field: unpadded point i holds density (copy) or its trilinear sample at
    g = a + i * s, and iso - 1 where the occupancy mask (looked up at mn + i * h) is 0."""
    density = np.asarray(density, f32)
    ii = [np.arange(n, dtype=f32) for n in R]
    I, J, K = np.meshgrid(*ii, indexing='ij')
    if copy:
        vals = density.copy()
    else:
        a, s = np.asarray(a, f32), np.asarray(s, f32)
        vals = trilinear(density, a[0] + I * s[0], a[1] + J * s[1], a[2] + K * s[2])
    occ = None
    if mask is not None:
        mn, h = np.asarray(mn, f32), np.asarray(h, f32)
        sc, sh = np.asarray(mask_scale, f32), np.asarray(mask_shift, f32)
        idx = []
        for ax, G in enumerate((I, J, K)):
            x = _fma32(mn[ax] + G * h[ax], sc[ax], sh[ax])
            idx.append((np.sign(x) * np.floor(np.abs(x) + f32(0.5))).astype(np.int64))   # roundf: half away from zero
        ok = np.ones(I.shape, bool)
        for ax in range(3):
            ok &= (idx[ax] >= 0) & (idx[ax] < mask.shape[ax])
        occ = ok & np.asarray(mask, bool)[tuple(np.clip(idx[ax], 0, mask.shape[ax] - 1) for ax in range(3))]
    return pad_field(vals, iso, occ)


def _grad(F, h):
    G = np.empty(F.shape + (3,), f32)
    for ax in range(3):
        n = F.shape[ax]
        up = np.take(F, np.minimum(np.arange(n) + 1, n - 1), axis=ax)
        dn = np.take(F, np.maximum(np.arange(n) - 1, 0), axis=ax)
        G[..., ax] = (up - dn) / f32(h[ax])
    return G


def crossings(F, iso):
    """[N, 7] bool: the edge from point n (linear order) in direction d crosses the surface"""
    P = F.shape
    inside = F > f32(iso)
    cross = np.zeros((7,) + P, bool)
    for d, (bx, by, bz) in enumerate(DIRS):
        cross[d, :P[0] - bx, :P[1] - by, :P[2] - bz] = (inside[:P[0] - bx, :P[1] - by, :P[2] - bz]
                                                       != inside[bx:, by:, bz:])
    return cross.reshape(7, F.size).T


def vertex_edges(F, iso):
    """(padded lattice point [V,3], direction [V]) of every vertex, in id order"""
    pts, dirs = np.nonzero(crossings(F, iso))               # point order, then direction order
    return np.stack(np.unravel_index(pts, F.shape), 1), dirs


def marching_tets(F, iso, mn, h):
    F = np.asarray(F, f32)
    iso, mn, h = f32(iso), np.asarray(mn, f32), np.asarray(h, f32)
    P = F.shape
    N = F.size
    inside = F > iso
    cf = crossings(F, iso)
    ids = np.cumsum(cf.ravel()).reshape(N, 7) - 1               # id of (point, direction) where it crosses
    pts, dirs = np.nonzero(cf)
    V = len(pts)

    # vertices and normals
    pijk = np.stack(np.unravel_index(pts, P), 1)
    e = DIRS[dirs]
    qijk = pijk + e
    f0 = F[tuple(pijk.T)]
    f1 = F[tuple(qijk.T)]
    t = (iso - f0) / (f1 - f0)
    verts = np.empty((V, 3), f32)
    for ax in range(3):
        verts[:, ax] = mn[ax] + ((pijk[:, ax] - 1).astype(f32) + t * e[:, ax].astype(f32)) * h[ax]
    G = _grad(F, h)
    g0, g1 = G[tuple(pijk.T)], G[tuple(qijk.T)]
    g = g0 + t[:, None] * (g1 - g0)
    ln = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
    nz = ln > 0
    normals = np.zeros((V, 3), f32)
    normals[nz] = -g[nz] / ln[nz, None]

    # faces: only cells with corners on both sides
    c_in = inside[:-1, :-1, :-1].copy()
    c_any, c_all = c_in.copy(), c_in.copy()
    corner = {}
    for off in itertools.product((0, 1), repeat=3):
        s = inside[off[0]:P[0] - 1 + off[0], off[1]:P[1] - 1 + off[1], off[2]:P[2] - 1 + off[2]]
        corner[off] = s
        c_any |= s
        c_all &= s
    cells = np.stack(np.nonzero(c_any & ~c_all), 1)               # lower corners, lexicographic = point order
    cell_lin = np.ravel_multi_index(tuple(cells.T), P)
    tab = case_table()
    keys, tris = [], []
    for t_i, perm in enumerate(PERMS):
        cs = tet_corners(perm)
        case = np.zeros(len(cells), np.int64)
        for k, c in enumerate(cs):
            case |= corner[tuple(c)][tuple(cells.T)].astype(np.int64) << k
        for m in range(1, 15):
            poly = tab[(t_i, m)]
            sel = np.nonzero(case == m)[0]
            if not poly or not len(sel):
                continue
            q = [ids[np.ravel_multi_index(tuple((cells[sel] + np.array(lo)).T), P), d] for lo, d in poly]
            if len(q) == 3:
                keys.append(np.stack([cell_lin[sel], np.full(len(sel), t_i), np.zeros(len(sel), np.int64)], 1))
                tris.append(np.stack(q, 1))
            else:
                q0, q1, q2, q3 = q
                diag02 = np.minimum(q0, q2) < np.minimum(q1, q3)
                ta = np.where(diag02[:, None], np.stack([q0, q1, q2], 1), np.stack([q0, q1, q3], 1))
                tb = np.where(diag02[:, None], np.stack([q0, q2, q3], 1), np.stack([q1, q2, q3], 1))
                for r, tr in enumerate((ta, tb)):
                    keys.append(np.stack([cell_lin[sel], np.full(len(sel), t_i), np.full(len(sel), r)], 1))
                    tris.append(tr)
    if not tris:
        return verts, np.zeros((0, 3), np.int32), normals
    keys = np.concatenate(keys)
    tris = np.concatenate(tris)
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    return verts, tris[order].astype(np.int32), normals


# ------------------------------------------------------------------------------------------------ mesh checks
def canonical_faces(faces):
    """each triangle rotated so that its smallest id comes first (orientation kept), rows sorted"""
    f = np.asarray(faces, np.int64)
    r = np.argmin(f, 1)
    idx = (r[:, None] + np.arange(3)[None]) % 3
    g = np.take_along_axis(f, idx, 1)
    return g[np.lexsort((g[:, 2], g[:, 1], g[:, 0]))]


def half_edges_ok(faces):
    """(every undirected edge in exactly 2 faces, every directed half-edge exactly once)"""
    f = np.asarray(faces, np.int64)
    he = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    n = int(f.max()) + 1 if len(f) else 1
    d_codes = he[:, 0] * n + he[:, 1]
    u_codes = np.minimum(he[:, 0], he[:, 1]) * n + np.maximum(he[:, 0], he[:, 1])
    _, dc = np.unique(d_codes, return_counts=True)
    _, uc = np.unique(u_codes, return_counts=True)
    return bool((uc == 2).all()), bool((dc == 1).all())


def euler_characteristic(n_verts, faces):
    f = np.asarray(faces, np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e = np.unique(np.sort(e, 1), axis=0)
    return int(n_verts) - len(e) + len(f)


def area_and_volume(verts, faces):
    v = np.asarray(verts, np.float64)
    a, b, c = (v[np.asarray(faces)[:, k]] for k in range(3))
    cr = np.cross(b - a, c - a)
    return 0.5 * np.linalg.norm(cr, axis=1).sum(), (a * cr).sum() / 6.0
