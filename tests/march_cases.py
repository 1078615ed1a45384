"""The edge-case table of the fused march (test infrastructure, CPU only; used by tests/test_march_oracle_host.py and
tests/test_gpu_march_oracle.py).

Scenes are built by hand so that the density at step s of a ray is chosen, not found.  Lattice X x 9 x 9 with spacing h =
2^-6, xyz_min = 0, X - 1 a power of two: the voxel coordinates of a point on a lattice line are exact in float32
(`dvgo_src_index` divides by 8 h and by (X - 1) h).  Each of the lines (j, k), j, k < 8, along x carries its own density profile and
its own occupancy column; a ray along +x from (-2 h, j h, k h) with near = 0 starts on the face x = 0, takes 2 (X - 1) steps
of half a voxel (stepsize 0.5) and sees only its own line: even steps on a voxel, odd steps half way between two (the other
lines enter with weight exactly 0).  A ray along a line with j == 8 or k == 8 lies in the upper face, where the slab test of
`dvgo_ray_setup` gives t_max == t_min (n_steps == 1: the reference's behaviour): such a ray has the one sample of row 'on-xyz_max'.  act_shift and interval are what DirectVoxGO sets for alpha_init (1e-2 fine, 1e-6
coarse) and stepsize 0.5 at voxel_size_ratio 1.

Density levels (alpha_init = 1e-2, act_shift = -4.5951, interval 0.5):
    AIR  -40     alpha == 0.0f exactly (1 + e rounds to 1), also half way between AIR and anything below 0
    FOG  -0.9234 alpha ~ 0.002: kept by both filters for hundreds of steps (0.998^513 = 0.36)
    WEAK -2.3119 alpha ~ 5e-4: above thres = 1e-4, its weight below once T < 0.2
    HALF  5.6937 alpha ~ 0.5      SEMI 9.190 alpha ~ 0.9
    EDGE 37.87   alpha == 1 - 2^-24 (p = (1 + e)^-0.5 ~ 2^-24, the float below 1)
    WALL 60      alpha == 1.0f, e ~ 1e24 (> 1e10); half way FOG / WALL: e ~ 6.5e10, alpha ~ 1 - 4e-6: the ray stops there
    INF  100     e == inf
Every decision a row relies on has a margin far above the activation's allowance (exp2 / log2 against powf, 1e-5), or is
exact on both sides (alpha == 0, alpha == 1).

Rows: (name, target, predicate).  The predicate takes a `Result` -- the CPU oracle's in the host test, the device's in the
GPU test -- and must hold for the row to count.  Rows of the issue's table that cannot be built through `fused_march`:
    n_steps == 0            `dvgo_ray_setup` returns max(ceil(.), 1): a ray that misses the box has n_steps == 1 (row 'miss')
    n_steps == rec_stride   rec_stride = ceil((far - near) / stepdist) + 2 > n_steps always
    record dropped by the weight filter as the FIRST of a ray: its T is 1, so its weight is its alpha > thres
    n3 == 0 with n2 > 0     for the same reason; n3 == 0 is covered with n2 == 0
"""
import numpy as np

import march_oracle as M

H = 2.0 ** -6
AIR, FOG, WEAK, HALF, SEMI, EDGE, WALL, INF = -40.0, -0.9234, -2.3119, 5.6937, 9.190, 37.87, 60.0, 100.0
_F = np.float32


class Scene:
    """One lattice and a batch of rays.  `lines`: {(j, k): (profile [X], occupancy [X] bool or None)}; other lines are AIR."""

    def __init__(self, name, X, alpha_init, thres, C, ndc=0):
        self.name, self.X, self.thres, self.C, self.ndc = name, X, thres, C, ndc
        self.act_shift = 0.0 if ndc else float(np.log(1 / (1 - alpha_init) - 1))
        self.interval, self.stepdist = 0.5, 0.5 * H
        self.xyz_min = np.zeros(3, np.float32)
        self.xyz_max = np.array([(X - 1) * H, 8 * H, 8 * H], np.float32)
        self.density = np.full((X, 9, 9), AIR, np.float32)
        self.mask = np.ones((X, 9, 9), bool)
        self.near, self.far = 0.0, float((X - 1) * H + 8 * H)
        self.rays, self.rows = [], []

    def line(self, j, k, profile, occ=None):
        self.density[:, j, k] = profile
        if occ is not None:
            self.mask[:, j, k] = occ

    def ray(self, o, d):
        self.rays.append((o, d))
        return len(self.rays) - 1

    def along_x(self, j, k):
        return self.ray((-2 * H, j * H, k * H), (1.0, 0.0, 0.0))

    def row(self, name, target, pred):
        self.rows.append((name, target, pred))

    def arrays(self):
        o = np.array([r[0] for r in self.rays], np.float32)
        d = np.array([r[1] for r in self.rays], np.float32)
        return o, d

    @property
    def mask_scale(self):
        return ((np.array(self.mask.shape, np.float32) - _F(1)) / (self.xyz_max - self.xyz_min)).astype(np.float32)

    @property
    def mask_shift(self):
        return (-self.xyz_min * self.mask_scale).astype(np.float32)


class Result:
    """What a predicate sees: R (march_oracle.Records), n2, n3, last, n_steps [N]; rays_start [N, 3] when known."""

    def __init__(self, R, n3, last, n_steps, start=None):
        self.R, self.n2, self.n3, self.last, self.n_steps, self.start = R, R.n, np.asarray(n3, np.int64), last, np.asarray(n_steps, np.int64), start

    def steps(self, r):
        return self.R.step[self.R.first[r]:self.R.first[r + 1]]

    def of(self, r, what):
        return getattr(self.R, what)[self.R.first[r]:self.R.first[r + 1]]

    def stopped_at(self, r):
        """step of the record that stopped ray r, or None"""
        return int(self.steps(r)[-1]) if self.n2[r] and float(self.last[r]) < 1e-3 else None


def cpu_forward(sc, O):
    """The forward of `sc` on the C oracle (oracle/dvgo_oracle.c) in the reference's op order -> Result."""
    o, d = sc.arrays()
    N = o.shape[0]
    if sc.ndc:
        pts, out = O.sample_ndc_pts_on_rays(o, d, sc.xyz_min, sc.xyz_max, sc.ndc)
        keep = ~out
        ray_id = np.broadcast_to(np.arange(N, dtype=np.int64)[:, None], keep.shape)[keep]
        step_id = np.broadcast_to(np.arange(sc.ndc, dtype=np.int64)[None, :], keep.shape)[keep]
        pts, n_steps, start = pts[keep], np.full(N, sc.ndc, np.int64), o
    else:
        pts, out, ray_id, step_id, n_steps, t_min, _ = O.sample_pts_on_rays(o, d, sc.xyz_min, sc.xyz_max, sc.near, sc.far, float(_F(sc.stepdist)))
        pts, ray_id, step_id = pts[~out], ray_id[~out], step_id[~out]
        start = O.infer_ray_start_dir(o, d, t_min)[0]
    sel = O.maskcache_lookup(sc.mask, pts, sc.mask_scale, sc.mask_shift)
    pts, ray_id, step_id = pts[sel], ray_id[sel], step_id[sel]
    dens = O.grid_sample_fwd(sc.density[None], pts, sc.xyz_min, sc.xyz_max, use_fma=True)[:, 0]
    with np.errstate(all='ignore'):
        exp_d, alpha = O.raw2alpha(dens, sc.act_shift, sc.interval)
    if sc.thres > 0:
        sel = alpha > _F(sc.thres)
        ray_id, step_id, exp_d, alpha = ray_id[sel], step_id[sel], exp_d[sel], alpha[sel]
    w, T, last, i_start, i_end = O.alpha2weight(alpha, ray_id, N)
    n2 = i_end - i_start
    rows = np.concatenate([np.arange(a, b) for a, b in zip(i_start, i_end)]) if N else np.zeros(0, np.int64)
    rows = rows.astype(np.int64)
    flag = (w[rows] > _F(sc.thres)) if sc.thres > 0 else np.ones(rows.shape[0], bool)
    s = (step_id[rows].astype(np.int64) | np.where(flag, 1 << 31, 0)).astype(np.uint32).view(np.int32)
    rec2 = np.stack([s.view(np.float32), exp_d[rows], alpha[rows], T[rows]], 1)
    R = M.Records(rec2, n2, np.concatenate([[0], np.cumsum(n2)])[:-1])
    return Result(R, np.bincount(R.ray, R.flag, N), last, n_steps, start)


def _stop_profile(X, s):
    """a profile on which the ray stops at step s exactly (module text: odd steps stop half way FOG / WALL; for an even
    step the voxel before the wall is AIR, so that the half-way sample there (d = 10, alpha ~ 0.93) does not stop)"""
    v = np.full(X, FOG, np.float32)
    if s % 2:
        v[(s + 1) // 2:] = WALL
    else:
        v[s // 2:] = WALL
        if s >= 2:
            v[s // 2 - 1] = AIR
    return v


def _fog_until(X, m):
    v = np.full(X, AIR, np.float32)
    v[:m + 1] = FOG
    return v


def _hole0(X):
    occ = np.ones(X, bool)
    occ[0] = False
    return occ


def fine_scene():
    """X = 129 (256 steps, four chunks), alpha_init 1e-2, thres 1e-4, 12 feature channels."""
    sc = Scene('fine129', 129, 1e-2, 1e-4, 12)
    X = sc.X
    lines = [(j, k) for j in range(8) for k in range(8)]
    empty = lines[15]
    r_first = sc.along_x(*empty)                               # ray 0 of the batch has no sample
    for n, s in enumerate((0, 1, 62, 63, 64, 65, 126, 127, 192, 193, 254, 255)):
        sc.line(*lines[n], _stop_profile(X, s))
        r = sc.along_x(*lines[n])
        sc.row(f'stop@{s}', f'early stop on lane {s % 64} of chunk {s // 64}' + (' (the ray\'s last step)' if s == 255 else ''),
               lambda q, r=r, s=s: q.stopped_at(r) == s and q.n_steps[r] == 256)
    sc.line(*lines[30], np.full(X, FOG, np.float32))
    sc.line(8, 8, np.full(X, FOG, np.float32))                # (the line on xyz_max in y and z: row 'on-xyz_max')
    r = sc.r_never = sc.along_x(*lines[30])
    sc.row('never', 'ray that never stops', lambda q, r=r: q.last[r] >= 1e-3 and q.n2[r] == 256 and q.steps(r)[-1] == q.n_steps[r] - 1)
    v = np.full(X, FOG, np.float32); v[11:81] = AIR
    sc.line(*lines[13], v)
    r = sc.along_x(*lines[13])
    sc.row('gap-alpha', 'chunks with no kept lane between kept chunks, alpha below the threshold',
           lambda q, r=r: np.diff(q.steps(r)).max() > 128 and q.steps(r)[-1] > 200)
    occ = np.ones(X, bool); occ[20:61] = False
    sc.line(*lines[14], np.full(X, FOG, np.float32), occ)
    r = sc.along_x(*lines[14])
    sc.row('gap-mask', 'a chunk with no kept lane between kept chunks, hole in the occupancy mask',
           lambda q, r=r: np.diff(q.steps(r)).max() > 64 and q.steps(r)[-1] == 255)
    for n, (n2, m, hole) in enumerate(((1, 0, False), (63, 31, False), (64, 32, True), (65, 32, False), (128, 64, True), (129, 64, False))):
        sc.line(*lines[16 + n], _fog_until(X, m), _hole0(X) if hole else None)
        r = sc.along_x(*lines[16 + n])
        sc.row(f'n2={n2}', f'n2 == n3 == {n2}', lambda q, r=r, n2=n2: q.n2[r] == n2 and q.n3[r] == n2)
    v = np.full(X, AIR, np.float32); v[:6] = FOG; v[8] = EDGE
    sc.line(*lines[22], v)
    r = sc.along_x(*lines[22])
    sc.row('alpha=1-2^-24', 'alpha == 1 - 2^-24 (1 - alpha == 2^-24)', lambda q, r=r: q.of(r, 'alpha')[-1] == _F(1) - _F(2.0 ** -24) and q.stopped_at(r) == 16)
    sc.line(*lines[23], np.full(X, INF, np.float32))
    r = sc.along_x(*lines[23])
    sc.row('exp=inf', 'exp_d == inf, alpha == 1.0f on the first step', lambda q, r=r: np.isinf(q.of(r, 'exp_d')[0]) and q.of(r, 'alpha')[0] == 1 and q.n2[r] == 1)
    v = np.full(X, AIR, np.float32); v[0] = SEMI; v[1:5] = WEAK; v[5] = HALF; v[6:9] = WEAK
    sc.line(*lines[12], v)
    r = sc.along_x(*lines[12])
    sc.row('weight-filter', 'records kept by the alpha filter and dropped by the weight filter, in the middle and as the last of a ray',
           lambda q, r=r: (lambda f, a: (not f[-1]) and (not f[3]) and f[0] and f[10] and a.min() > 1e-4 and 0 < q.n3[r] < q.n2[r])(q.of(r, 'flag'), q.of(r, 'alpha')))
    r_wall = 1                                                  # stop@0: alpha == 1.0f, exp_d > 1e10
    sc.row('alpha=1', 'alpha == 1.0f (1 - alpha == 0: denominator 1e-10), exp_d > 1e10', lambda q: q.of(r_wall, 'alpha')[0] == 1 and 1e10 < q.of(r_wall, 'exp_d')[0] < np.inf)
    sc.row('empty-first', 'every sample dropped next to normal rays; ray 0 of the batch', lambda q: q.n2[r_first] == 0 and q.last[r_first] == 1 and q.n3[r_first] == 0)
    # ---- ray geometry
    fin = lambda q, r: bool(np.all(np.isfinite(q.start[r]))) and q.n_steps[r] > 0
    r = sc.ray(((X + 1) * H, 1 * H, 1 * H), (-1.0, 0.0, 0.0))
    sc.row('-x', 'axis-parallel ray, two zero direction components, negative sign', lambda q, r=r: fin(q, r) and q.n2[r] > 0)
    r = sc.ray((-2 * H, 1 * H, 1 * H), (1.0, 0.01, 0.0))
    sc.row('tilt-y', 'one zero direction component', lambda q, r=r: fin(q, r) and q.n2[r] > 0)
    r = sc.ray((-2 * H, lines[30][0] * H, lines[30][1] * H), (1.0, -0.01, 0.004))
    sc.row('tilt-yz', 'tilted ray, no zero component', lambda q, r=r: fin(q, r) and q.n2[r] > 0)
    r = sc.ray((10 * H, -2 * H, 2 * H), (0.0, 1.0, 0.0))
    sc.row('+y', 'axis-parallel ray along +y (16 steps)', lambda q, r=r: fin(q, r) and q.n_steps[r] == 16)
    r = sc.ray((10 * H, 2 * H, 10 * H), (0.0, 0.0, -2.0))
    sc.row('-z', 'axis-parallel ray along -z, direction of length 2 (the step count is taken in units of |d|, as the reference does)', lambda q, r=r: fin(q, r) and q.n_steps[r] == 8)
    r = sc.ray((10.25 * H, lines[30][0] * H, lines[30][1] * H), (1.0, 0.0, 0.0))
    sc.row('inside', 'origin inside the box', lambda q, r=r: fin(q, r) and q.start[r][0] == _F(10.25 * H) and q.n2[r] > 0)
    r = sc.ray((0.0, 2 * H, 2 * H), (1.0, 0.0, 0.0))
    sc.row('on-face', 'origin on a face of the box', lambda q, r=r: fin(q, r) and q.start[r][0] == 0 and q.n_steps[r] == 256)
    r = sc.ray((-2 * H, 12 * H, 2 * H), (1.0, 0.0, 0.0))
    sc.row('miss', 'ray that misses the box: n_steps == 1, no sample', lambda q, r=r: q.n_steps[r] == 1 and q.n2[r] == 0)
    r = sc.ray(((X + 1) * H, 8 * H, 8 * H), (-1.0, 0.0, 0.0))
    sc.row('on-xyz_max', 'samples exactly on xyz_max: upper corners outside the lattice',
           lambda q, r=r: q.n2[r] > 0 and q.steps(r)[0] == 0 and corners_in_range(sc, q, r).max() < 8 and corners_in_range(sc, q, r)[0] == 1)
    r_min = sc.along_x(0, 0)
    sc.row('on-xyz_min', 'samples exactly on xyz_min in y and z: floor corner 0, weight of the upper corners exactly 0',
           lambda q: q.n2[r_min] > 0 and corners_in_range(sc, q, r_min).min() == 8)
    r_last = sc.along_x(*empty)                                 # the last ray of the batch has no sample either
    sc.row('empty-last', 'the last ray of the batch has no sample', lambda q: q.n2[r_last] == 0 and q.last[r_last] == 1 and r_last == len(sc.rays) - 1)
    return sc


def corners_in_range(sc, q, r):
    """number of in-range corners of every record of ray r (brick_oracle.tri_setup on the ray's own start and direction)"""
    import brick_oracle as B
    o, d = sc.arrays()
    dirs = (d[r] / np.sqrt(np.float32((d[r].astype(np.float64) ** 2).sum()))).astype(np.float32)
    steps = q.steps(r)
    recs = np.stack([np.zeros_like(steps), np.zeros_like(steps), steps, np.zeros_like(steps)], 1).astype(np.int32)
    p = B.positions(recs, q.start[r][None], dirs[None], sc.stepdist)
    return B.tri_setup(p, sc.xyz_min, sc.xyz_max, sc.X, 9, 9)[2].sum(1)


def long_scene():
    """X = 1025 (2048 steps): the record counts around march_composite's round of 256 and beyond 512."""
    sc = Scene('fine1025', 1025, 1e-2, 1e-4, 12)
    X = sc.X
    lines = [(j, k) for j in range(8) for k in range(8)]
    for n, (n3, m, hole) in enumerate(((255, 127, False), (256, 128, True), (257, 128, False), (513, 256, False), (64, 32, True), (1, 0, False))):
        sc.line(*lines[n], _fog_until(X, m), _hole0(X) if hole else None)
        r = sc.along_x(*lines[n])
        sc.row(f'n3={n3}', f'n3 == n2 == {n3}', lambda q, r=r, n3=n3: q.n3[r] == n3 and q.n2[r] == n3)
    r = sc.along_x(*lines[20])
    sc.row('n3=0', 'n3 == 0 (no record at all: see the module text)', lambda q, r=r: q.n3[r] == 0 and q.n2[r] == 0)
    for n, s in enumerate((1280, 1343, 2047)):
        sc.line(*lines[6 + n], _stop_profile(X, s))
        r = sc.along_x(*lines[6 + n])
        sc.row(f'stop@{s}', f'early stop on lane {s % 64} of chunk {s // 64}', lambda q, r=r, s=s: q.stopped_at(r) == s)
    sc.line(*lines[9], np.full(X, FOG, np.float32))
    r = sc.along_x(*lines[9])
    sc.row('long-never', '2048 records, never stops; the tail falls below the weight filter',
           lambda q, r=r: q.n2[r] == 2048 and q.last[r] >= 1e-3 and 513 < q.n3[r] < 2048 and not q.of(r, 'flag')[-1])
    return sc


def coarse_scene():
    """thres == 0 (the coarse stage: no filter, k0 = 3 colour channels, alpha_init 1e-6): alpha == 0.0f samples are kept."""
    sc = Scene('coarse129', 129, 1e-6, 0.0, 3)
    X = sc.X
    occ = np.ones(X, bool); occ[30:41] = False
    sc.line(1, 1, np.full(X, AIR, np.float32), occ)
    r = sc.along_x(1, 1)
    # steps 60 .. 80 round to the voxels 30 .. 40 (59 -> 29.5 -> 30 as well: roundf rounds half away from zero)
    sc.row('zeros-kept', 'thres == 0: alpha == 0.0f samples kept, T unchanged across them',
           lambda q, r=r: q.n2[r] == 256 - 22 and np.all(q.of(r, 'alpha') == 0) and np.all(q.of(r, 'T') == 1) and q.last[r] == 1 and q.n3[r] == q.n2[r])
    v = np.full(X, 0.0, np.float32); v[40:60] = AIR
    sc.line(2, 2, v)
    r = sc.along_x(2, 2)
    sc.row('zeros-between', 'thres == 0: a run of alpha == 0.0f between samples with alpha > 0',
           lambda q, r=r: q.n2[r] == 256 and (q.of(r, 'alpha') == 0).sum() > 30 and q.of(r, 'alpha')[0] > 0 and q.of(r, 'alpha')[-1] > 0)
    sc.line(3, 3, _stop_profile(X, 127))
    r = sc.along_x(3, 3)
    sc.row('coarse-stop', 'thres == 0: early stop on lane 63 of chunk 1', lambda q, r=r: q.stopped_at(r) == 127 and q.n2[r] == 128)
    r = sc.along_x(0, 4)
    sc.row('coarse-air', 'thres == 0: n2 == number of in-box unmasked steps', lambda q, r=r: q.n2[r] == 256 and q.n3[r] == 256)
    return sc


def ndc_scene(n_samples):
    """NDC / MPI spacing (stepdist < 0): rays_o on the face x = 0, un-normalised rays_d spanning the box, N_samples steps."""
    X = {64: 33, 65: 33, 129: 65}[n_samples]
    sc = Scene(f'ndc{n_samples}', X, 1e-2, 1e-4, 9, ndc=n_samples)
    v = np.full(X, -6.0, np.float32); v[X // 2:] = -4.0
    sc.density[:] = v[:, None, None]                           # density depends on x only
    span = (X - 1) * H
    r = sc.ray((0.0, 1 * H, 1 * H), (span, 0.0, 0.0))
    sc.row('ndc-axis', f'N_samples == {n_samples}, every sample a record', lambda q, r=r: q.n_steps[r] == n_samples and q.n2[r] == n_samples)
    r = sc.ray((0.0, 2 * H, 3 * H), (span, 0.3 * H, -0.2 * H))
    sc.row('ndc-tilt', f'N_samples == {n_samples}, tilted', lambda q, r=r: q.n_steps[r] == n_samples and q.n2[r] == n_samples)
    r = sc.ray((0.0, 12 * H, 0.0), (span, 0.0, 0.0))
    sc.row('ndc-out', 'a ray outside the box: every step out', lambda q, r=r: q.n2[r] == 0)
    return sc


def nan_scene():
    """`fine129` with one NaN voxel on the never-stopping line (thres > 0: the filter drops every sample that reads it)."""
    sc = fine_scene()
    sc.name = 'fine129-nan'
    sc.density[40, 3, 6] = np.nan
    sc.rows = [('nan-dropped', 'one density voxel NaN with thres > 0: dropped by the filter, no NaN in any record',
                lambda q: not np.isnan(q.R.alpha).any() and not np.isnan(q.R.T).any() and not np.isnan(q.last).any() and q.n2[sc.r_never] < 256)]
    return sc


def all_scenes():
    return [fine_scene(), long_scene(), coarse_scene(), ndc_scene(64), ndc_scene(65), ndc_scene(129), nan_scene()]
