"""The edge-case table of the fused march over contracted space (csrc/march_contract.hip): test infrastructure, CPU only;
used by tests/test_march_contract_host.py and tests/test_gpu_march_contract.py.

Sizes are chosen by what can go wrong in a kernel that puts 64 consecutive table steps on the lanes of a wavefront:

  case       world step  b    norm  n_max  N   scene  mask        thres  what it is there for
  partial42  24    1.0   0.2  inf   42     7   wall   none        1e-4   one partial chunk; rays stopped inside the first chunk
  carry82    24    0.5   0.2  l2    82     65  fog    half-space  1e-4   the thinning's acc carried over the border at step 64
  three162   48    0.5   0.2  inf   162    65  fog    all true    0      three chunks, a stop in a later chunk, no filters
  b05_l2     24    0.5   0.5  l2    66     7   wall   none        0      a second chunk of two lanes; thres == 0 with a stop
  empty      24    1.0   0.2  inf   42     1   empty  all true    1e-4   every n2 == 0, one ray
  allfalse   24    0.5   0.2  inf   82     7   fog    all false   1e-4   every chunk skipped: the thinning walk alone
  b05_fog    48    0.5   0.5  inf   130    65  fog    half-space  1e-4   b = 0.5 with the max norm, an off-centre foreground box
  lengths    80    0.5   0.2  inf   268    6   haze   per-sample  1e-4   rays of exactly 1, 63, 64, 65, 129 and 0 records

Rays (normalised coordinates, mapped through the case's centre and radius): origin inside the unit box; origin in the shell,
pointing inward; along an axis through the origin; with |x| == |y| (ties of the max norm); grazing n == 1 along a face of the
unit box; leaving through a corner and never re-entering; then random ones.  N == 1 takes the first, N == 7 the six and one
random ray.

Scenes are raw densities within +-20, with act_shift = 0 and interval = stepsize, so every reference quantity is finite:
empty -20; wall +20 outside max|q| = 0.5 and -20 inside; fog about -1.5 (alpha about 0.1: the stop falls 50 to 70 records in);
haze about -3 (never stops), all with a little noise so that the trilinear read matters.  `cpu_forward` restates the march in
numpy (alpha through np.power, not the device's exp2 / log2: good for the counts and the stop steps the table is about, not for
bits) so that the host test can say every case hits its edge.
"""
import numpy as np

import unbounded_oracle as U

f32 = np.float32

TABLE = {  # name: (world, stepsize, b, norm, n_max, N, scene, mask, thres)
    'partial42': (24, 1.0, 0.2, 'inf', 42, 7, 'wall', 'none', 1e-4),
    'carry82': (24, 0.5, 0.2, 'l2', 82, 65, 'fog', 'half', 1e-4),
    'three162': (48, 0.5, 0.2, 'inf', 162, 65, 'fog', 'true', 0.0),
    'b05_l2': (24, 0.5, 0.5, 'l2', 66, 7, 'wall', 'none', 0.0),
    'empty': (24, 1.0, 0.2, 'inf', 42, 1, 'empty', 'true', 1e-4),
    'allfalse': (24, 0.5, 0.2, 'inf', 82, 7, 'fog', 'false', 1e-4),
    'b05_fog': (48, 0.5, 0.5, 'inf', 130, 65, 'fog', 'half', 1e-4),
    'lengths': (80, 0.5, 0.2, 'inf', 268, 6, 'haze', 'lengths', 1e-4),
}
LENGTHS = (1, 63, 64, 65, 129, 0)
LENGTHS_MASK = (1200, 8, 2)             # finer along x than the sample spacing: one voxel per sample


def special_rays():
    o = f32([[0.1, -0.2, 0.05], [1.8, 0.3, -0.4], [0.0, 0.0, 0.0], [0.2, 0.2, 0.0], [1.0, -0.9, 0.3], [0.5, 0.5, 0.5]])
    d = f32([[0.3, 0.8, -0.5], [-1.0, 0.1, 0.2], [1.0, 0.0, 0.0], [1.0, -1.0, 0.0], [0.0, 1.0, 0.0], [1.0, 1.0, 1.0]])
    return o, d


def rays(N, seed):
    o, d = special_rays()
    if N > o.shape[0]:
        rng = np.random.default_rng(seed)
        n = N - o.shape[0]
        ro = rng.uniform(-1.6, 1.6, (n, 3)).astype(f32)
        rd = rng.normal(size=(n, 3)).astype(f32)
        rd[::4, 0] = 0
        rd[np.abs(rd).max(-1) == 0, 2] = 1.0
        o, d = np.concatenate([o, ro]), np.concatenate([d, rd])
    return np.ascontiguousarray(o[:N]), np.ascontiguousarray(d[:N])


class Case:
    def __init__(self, name):
        self.name = name
        self.world, self.stepsize, self.b, self.norm, self.n_max, self.N, self.scene, self.mask_kind, self.thres = TABLE[name]
        W = self.world
        self.center = f32([0.3, -0.2, 0.1] if name == 'b05_fog' else [0, 0, 0])
        self.radius = f32([1.5, 0.8, 1.2] if name == 'b05_fog' else [1, 1, 1])
        self.act_shift, self.interval = 0.0, float(self.stepsize)
        lim = f32(1 + self.b)
        self.xyz_min, self.xyz_max = np.full(3, -lim, f32), np.full(3, lim, f32)
        self.t_tab, _, n_max = U.t_table(W, self.stepsize, self.b)
        assert n_max == self.n_max
        self.thin = U.threshold(W, self.stepsize, self.b)
        if name == 'lengths':
            o = np.zeros((6, 3), f32)
            o[:, 0] = -0.999
            o[:, 1] = np.linspace(-0.7, 0.7, 6)            # one row of the mask per ray
            o[:, 2] = 0.05
            d = np.tile(f32([1, 0, 0]), (6, 1))
        else:
            o, d = rays(self.N, seed=len(name))
        self.rays_o = (o * self.radius + self.center).astype(f32)
        self.rays_d = (d * self.radius).astype(f32)
        # density: raw values within +-20
        rng = np.random.default_rng(7)
        ax = np.linspace(-float(lim), float(lim), W)
        gx, gy, gz = np.meshgrid(ax, ax, ax, indexing='ij')
        noise = rng.normal(size=(W, W, W)) * 0.2
        if self.scene == 'empty':
            dens = np.full((W, W, W), -20.0)
        elif self.scene == 'wall':
            dens = np.where(np.maximum(np.maximum(np.abs(gx), np.abs(gy)), np.abs(gz)) > 0.5, 20.0, -20.0) + noise
        elif self.scene == 'fog':
            dens = -1.5 + noise
        else:
            dens = -3.0 + noise
        self.density = np.clip(dens, -20, 20).astype(f32)
        # occupancy
        mshape = LENGTHS_MASK if self.mask_kind == 'lengths' else (W, W, W)
        if self.mask_kind == 'none':
            self.mask = None
        elif self.mask_kind == 'true':
            self.mask = np.ones(mshape, bool)
        elif self.mask_kind == 'false':
            self.mask = np.zeros(mshape, bool)
        elif self.mask_kind == 'half':
            self.mask = np.zeros(mshape, bool)
            self.mask[: W // 2 + 3] = True                 # the half-space x below a plane just beyond the centre
        if self.mask_kind != 'none':
            # MaskCache's float32 expressions
            self.mask_scale = ((f32(mshape) - f32(1)) / (self.xyz_max - self.xyz_min)).astype(f32)
            self.mask_shift = (-self.xyz_min * self.mask_scale).astype(f32)
        else:
            self.mask_scale = self.mask_shift = None
        if self.mask_kind == 'lengths':
            self.mask = self._lengths_mask(mshape)

    def _lengths_mask(self, mshape):
        """occupied exactly at the voxels of the first LENGTHS[r] samples of ray r (the rays lie inside the unit box for all
        of the table's uniform half, where every step is kept, and no two samples share a voxel)"""
        q, ray_id, step_id, _, _ = U.sample(self.rays_o, self.rays_d, self.center, self.radius, self.world, self.stepsize, self.b,
                                            self.norm)
        mask = np.zeros(mshape, bool)
        for r, n in enumerate(LENGTHS):
            qr = q[ray_id == r][:n].astype(np.float64)
            assert qr.shape[0] == n
            ijk = np.rint(qr * self.mask_scale.astype(np.float64) + self.mask_shift.astype(np.float64)).astype(int)
            assert len(set(map(tuple, ijk))) == n, 'two samples share a voxel of the mask'
            mask[ijk[:, 0], ijk[:, 1], ijk[:, 2]] = True
        return mask

    def candidates(self):
        """tests/unbounded_oracle.sample: the samples that pass the thinning and the occupancy (needs the CPU oracle built
        when the case has a mask) -> q [M,3], ray_id, step_id [M], t [M]"""
        return U.sample(self.rays_o, self.rays_d, self.center, self.radius, self.world, self.stepsize, self.b, self.norm,
                        self.mask, self.mask_scale, self.mask_shift)[:4]


def cases():
    return [Case(n) for n in TABLE]


def march_filters(alpha, ray_id, N, thres):
    """The march's filters on candidate samples with the alphas given (float32, ray-major): alpha > thres, the float32
    transmittance recurrence through a double product, the stop after the first T < 1e-3, bit 31 = T * alpha > thres.
    -> (rec [M] bool: the candidate is a record, flag [M] bool, T [M] float32 (of the records), last [N] float32)"""
    alpha = np.asarray(alpha, f32)
    thres = f32(thres)
    M = alpha.shape[0]
    rec, flag, T = np.zeros(M, bool), np.zeros(M, bool), np.ones(M, f32)
    last = np.ones(N, f32)
    off = U.segments(ray_id, N)
    for r in range(N):
        Tc = f32(1)
        for i in range(off[r], off[r + 1]):
            a = alpha[i]
            if thres > 0 and not a > thres:
                continue
            rec[i], T[i] = True, Tc
            flag[i] = (Tc * a > thres) if thres > 0 else True
            Tc = f32(np.float64(Tc) * (1.0 - np.float64(a) + 1e-10))
            if np.float64(Tc) < 1e-3:
                break
        last[r] = Tc
    return rec, flag, T, last


def cpu_forward(case):
    """numpy restatement -> dict(n_cand [N], n2 [N], n3 [N], stop_step [N] (-1: no stop), steps of the records)"""
    import torch
    q, ray_id, step_id, t = case.candidates()
    dens = U.trilinear64(torch.from_numpy(case.density.astype(np.float64))[None], torch.from_numpy(q.astype(np.float64)),
                         torch.from_numpy(case.xyz_min.astype(np.float64)), torch.from_numpy(case.xyz_max.astype(np.float64)))[:, 0].numpy()
    alpha = (1 - np.power(1 + np.exp(dens + case.act_shift), -case.interval)).astype(f32)
    rec, flag, T, last = march_filters(alpha, ray_id, case.N, case.thres)
    N = case.N
    stop = np.full(N, -1, np.int64)
    stopped = last.astype(np.float64) < 1e-3
    for r in np.nonzero(stopped)[0]:
        stop[r] = step_id[rec & (ray_id == r)][-1]
    return dict(n_cand=np.bincount(ray_id, minlength=N), n2=np.bincount(ray_id[rec], minlength=N),
                n3=np.bincount(ray_id[flag], minlength=N), stop_step=stop, step=step_id[rec], ray=ray_id[rec], alpha=alpha, last=last)
