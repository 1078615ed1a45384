"""Hand-built rays and sample lists for the contraction's ray gradient (test infrastructure), shared by
tests/test_contract_raygrad_host.py (float32 restatement against the bound) and tests/test_gpu_contract_raygrad.py (the two
kernel entries against the same bound).  W = 24, stepsize = 0.5: n_max = 82 at bg_len = 0.2, so a ray spans two chunks of 64
lanes; sample lists of length 0, 1, 63, 64, 65 and 82 (steps ascending, wrapping round the table where it is shorter).

The foreground box has centre (0, -0.2, 0.05) and the anisotropic half-size (1, 1.5, 0.75): x is left unscaled so that the
constructed rays reach their special values exactly in float32, which `build` asserts on the float32 forward.
"""
import numpy as np

import contract_raygrad_oracle as CR
import unbounded_oracle as U

f32 = np.float32
WORLD, STEPSIZE = 24, 0.5
CENTER = np.array([0.0, -0.2, 0.05], f32)
RADIUS = np.array([1.0, 1.5, 0.75], f32)
LENGTHS = (0, 1, 63, 64, 65, 82)
REC_STRIDE = 96
NAMED = ('inside', 'outside', 'axis', 'tie_xy', 'tie_xy_neg', 'tie_yz', 'n_one', 'zero_g')


def _ray(o_n, u):
    """World-space ray whose normalised origin is o_n and whose u = d / r is `u`."""
    return CENTER + np.asarray(o_n, f32) * RADIUS, np.asarray(u, f32) * RADIUS


def build(norm, b, seed=5):
    """-> dict rays_o, rays_d [N,3], ray_id, step_id [M] int64, off [N+1], g [M,3] float32, t_tab, n_max, named {name: ray}."""
    rng = np.random.default_rng(seed)
    t_tab, n_in, n_max = U.t_table(WORLD, STEPSIZE, b)
    k_one = n_in // 2                                       # the table's midpoint (2 k + 1) / n_in is 1 there
    assert t_tab[k_one] == f32(1.0)
    rays, steps, named = [], [], {}

    def add(o_n, u, ks, name=None):
        if name:
            named[name] = len(rays)
        rays.append(_ray(o_n, u))
        steps.append(np.sort(np.asarray(ks, np.int64)))

    wrap = lambda n, hi=n_max: np.arange(n) % hi            # noqa: E731
    add([0.1, -0.2, 0.05], [0.3, -0.5, 0.4], wrap(82, n_in // 4), 'inside')        # t < 0.5: every sample stays inner
    add([1.5, 0.3, -2.0], [0.2, 0.9, 0.4], wrap(82), 'outside')
    add([0.0, 0.25, 0.5], [1.0, 0.0, 0.0], wrap(65), 'axis')
    add([0.0, 0.0, 0.25], [1.0, 1.0, 0.0], wrap(64), 'tie_xy')                     # |p_x| == |p_y| at every step
    add([0.0, 0.0, 0.25], [1.0, -1.0, 0.0], wrap(63), 'tie_xy_neg')
    add([0.125, 0.0, 0.0], [0.0, 1.0, 1.0], np.arange(n_in, n_max), 'tie_yz')      # |p_y| == |p_z| > |p_x|
    add([0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [k_one - 1, k_one, k_one + 1], 'n_one')  # p = (t, 0, 0): n == 1 at k_one
    add([0.7, -0.4, 0.2], [-0.3, 0.8, 0.5], wrap(82), 'zero_g')
    while len(rays) < 48:
        i = len(rays)
        n = LENGTHS[i % len(LENGTHS)] if i < 32 else int(rng.integers(0, n_max + 1))
        ks = wrap(n) if i % 2 else rng.choice(n_max, size=min(n, n_max), replace=False)
        add(rng.uniform(-1.5, 1.5, 3), rng.normal(size=3) * rng.uniform(0.5, 2.0), ks)
    rays_o = np.stack([r[0] for r in rays]).astype(f32)
    rays_d = np.stack([r[1] for r in rays]).astype(f32)
    ray_id = np.concatenate([np.full(len(s), i, np.int64) for i, s in enumerate(steps)])
    step_id = np.concatenate(steps)
    off = np.searchsorted(ray_id, np.arange(len(rays) + 1)).astype(np.int64)
    g = rng.normal(size=(len(ray_id), 3)).astype(f32)
    g[ray_id == named['zero_g']] = 0
    case = dict(rays_o=rays_o, rays_d=rays_d, ray_id=ray_id, step_id=step_id, off=off, g=g, t_tab=t_tab, n_max=n_max,
                named=named, norm=norm, b=b, k_one=k_one)
    _check(case)
    return case


def _check(case):
    """The constructed properties hold on the float32 forward (else the case would test nothing)."""
    o, d, _ = CR.ray_setup(case['rays_o'], case['rays_d'], CENTER, RADIUS)
    p, n, inner, axis, _ = CR.points(o, d, case['t_tab'], case['b'], case['norm'], case['ray_id'], case['step_id'])
    rid, nm = case['ray_id'], case['named']
    sel = lambda name: rid == nm[name]                       # noqa: E731
    assert inner[sel('inside')].all() and not inner[sel('outside')].any()
    assert (p[sel('axis')][:, 1:] == f32([0.25, 0.5])).all()
    for name in ('tie_xy', 'tie_xy_neg'):
        q = p[sel(name)]
        assert (np.abs(q[:, 0]) == np.abs(q[:, 1])).all() and (np.abs(q[:, 0]) > np.abs(q[:, 2])).any()
    q = p[sel('tie_yz')]
    assert (np.abs(q[:, 1]) == np.abs(q[:, 2])).all() and (np.abs(q[:, 1]) > np.abs(q[:, 0])).all()
    assert (axis[sel('tie_yz')] == 1).all()
    one = sel('n_one') & (case['step_id'] == case['k_one'])
    assert one.sum() == 1 and n[one][0] == f32(1.0) and inner[one][0]
    lengths = set(np.diff(case['off']).tolist())
    assert set(LENGTHS) <= lengths


def records(case):
    """The same samples as the fused march's records -> rec2 [N * REC_STRIDE, 4] int32 (the step in field 0, bit 31 set on
    every other record as the march flags kept ones; the other three fields are not read), n2 [N] int32, off2 = off."""
    N = case['rays_o'].shape[0]
    rec = np.full((N * REC_STRIDE, 4), -1, np.int32)          # an unused slot would be a step past the table
    off = case['off']
    for r in range(N):
        ks = case['step_id'][off[r]:off[r + 1]].astype(np.int32)
        ks[1::2] |= np.int32(-2 ** 31)
        rec[r * REC_STRIDE:r * REC_STRIDE + len(ks), 0] = ks
    return rec, np.diff(off).astype(np.int32)
