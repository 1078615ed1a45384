"""CPU: tests/brick_oracle.py held to the things it restates, before any GPU test relies on it.

  * the float32 setup (position fmaf, dvgo_tri_setup / inb / weight) against oracle/dvgo_oracle.c, bit for bit;
  * the float64 sums against float64 autograd of torch's grid_sample;
  * the Adam rule against the reference's MaskedAdam fixture and oracle.adam_upd;
  * the (sample, brick) incidences on hand-built cases;
  * the checks themselves: they pass a float32 emulation of the kernel and fail value-only faults of the kind the suite
    exists for (one corner dropped, m of one voxel not updated, a float4-wide masked test);
  * the share of undetermined elements of every synthetic input the GPU tests launch.
"""
import numpy as np
import pytest
import torch

import brick_oracle as B
from conftest import load_golden

MN, MX = np.array([-1.0, -0.75, -1.25], np.float32), np.array([1.0, 1.25, 0.75], np.float32)
LATTICES = [(20, 23, 18), (20, 20, 20), (23, 23, 23), (17, 17, 17), (26, 26, 26), (160, 160, 160)]


def _points(dims, rng):
    """Every face, edge and corner of the box, brick faces / edges / corners, and random points."""
    pts = [np.array([(MN[a], 0.5 * (MN[a] + MX[a]) + 0.0137, MX[a])[(i // 3 ** a) % 3] for a in range(3)], np.float32)
           for i in range(27)]
    size1 = np.array(dims, np.float64) - 1
    for i in range(1, 8):                                   # lattice coordinate 8 (a brick boundary) on the chosen axes
        g = np.array([8.0 if (i >> a) & 1 else 3.3 + a for a in range(3)])
        for eps in (-1e-6, 0.0, 1e-6):
            pts.append((MN + (g + eps) / size1 * (MX.astype(np.float64) - MN)).astype(np.float32))
    g = rng.uniform(-0.01, 1.01, (60, 3))
    pts.extend((MN + g * (MX.astype(np.float64) - MN)).astype(np.float32))
    return np.stack(pts)


def _sample_recs(n, gd=None):
    recs = np.zeros((n, 4), np.int32)
    recs[:, 0], recs[:, 1] = np.arange(n), np.arange(n)
    recs[:, 3] = (np.ones(n, np.float32) if gd is None else gd.astype(np.float32)).view(np.int32)
    return recs


@pytest.mark.parametrize('dims', LATTICES[:5])
def test_one_sample_scatter_equals_the_c_oracle_bit_for_bit(dims, oracle):
    """A single contribution involves no summation: float32(w * g) of the restated setup == ora_grid_sample_bwd."""
    rng = np.random.default_rng(1)
    X, Y, Z = dims
    C = 3
    for p in _points(dims, rng):
        g = rng.standard_normal((1, C)).astype(np.float32)
        want = oracle.grid_sample_bwd(g, (C, X, Y, Z), p[None], MN, MX)
        O = B.scatter(_sample_recs(1), None, p[None], np.zeros((1, 3), np.float32), 0.5, MN, MX, g, C, X, Y, Z, by_sample=True)
        got = O.ref[:, :C].astype(np.float32).reshape(X, Y, Z, C)
        assert np.array_equal(np.moveaxis(got, -1, 0).view(np.int32), want.view(np.int32)), p


def test_setup_at_full_size_lattice_and_positions_follow_the_c_oracle(oracle):
    rng = np.random.default_rng(2)
    X, Y, Z = LATTICES[5]
    pts = _points((X, Y, Z), rng)
    g = rng.standard_normal((pts.shape[0], 1)).astype(np.float32)
    for i in range(pts.shape[0]):
        want = oracle.grid_sample_bwd(g[i:i + 1], (1, X, Y, Z), pts[i:i + 1], MN, MX)
        O = B.scatter(_sample_recs(1), None, pts[i:i + 1], np.zeros((1, 3), np.float32), 0.5, MN, MX, g[i:i + 1], 1, X, Y, Z, by_sample=True)
        assert np.array_equal(O.ref[:, 0].astype(np.float32).reshape(X, Y, Z), want[0])
    # positions: start + dir * (stepdist * step), one fmaf per axis, as ora_sample_pts_fill
    ro = rng.uniform(-3, 3, (64, 3)).astype(np.float32)
    rd = -ro + rng.uniform(-0.5, 0.5, (64, 3)).astype(np.float32)
    stepdist = 0.0123
    pts, _, ray_id, step_id, _, t_min, _ = oracle.sample_pts_on_rays(ro, rd, MN, MX, 0.2, 6.0, stepdist)
    start, dirs = oracle.infer_ray_start_dir(ro, rd, t_min)
    recs = np.zeros((pts.shape[0], 4), np.int32)
    recs[:, 1], recs[:, 2] = ray_id, step_id
    assert pts.shape[0] > 1000
    assert np.array_equal(B.positions(recs, start, dirs, stepdist).view(np.int32), pts.view(np.int32))
    # stepdist < 0 encodes the forward-facing sampling: dist = step / (n_samples - 1), as ora_sample_ndc_pts_on_rays
    n_samples = 37
    want, _ = oracle.sample_ndc_pts_on_rays(ro, rd, MN, MX, n_samples)
    recs = np.zeros((64 * n_samples, 4), np.int32)
    recs[:, 1], recs[:, 2] = np.repeat(np.arange(64), n_samples), np.tile(np.arange(n_samples), 64)
    got = B.positions(recs, ro, rd, -float(n_samples - 1))
    assert np.array_equal(got.view(np.int32), want.reshape(-1, 3).view(np.int32))
    # and the fma itself where double rounding would bite: exact ties of the float32 result
    a = np.float32(1 + 2.0 ** -23); b = np.float32(1 + 2.0 ** -23); c = np.float32(2.0 ** -60)
    assert B.fma32(a, b, c) == np.float32(np.float64(a) * np.float64(b))
    assert B.fma32(np.float32(1.0), np.float32(1 + 2.0 ** -23), np.float32(2.0 ** -24)) == np.float32(1 + 2.0 ** -22)
    assert B.fma32(np.float32(1.0), np.float32(1.0), np.float32(2.0 ** -24)) == np.float32(1.0)            # tie -> even
    assert B.fma32(np.float32(1 + 2.0 ** -23), np.float32(1 + 2.0 ** -23), np.float32(0)) == np.float32(1 + 2.0 ** -22)
    assert B.fma32(np.float32(1.0), np.float32(1.0), np.float32(2.0 ** -24 + 2.0 ** -47)) == np.float32(1 + 2.0 ** -23)   # just over


@pytest.mark.parametrize('dims', [(17, 17, 17), (33, 17, 9)])
def test_float64_sums_equal_float64_autograd_of_grid_sample(dims):
    """Box and positions chosen so that the float32 setup is exact (box edge and size - 1 powers of two, positions on
    a 1/64 grid): torch's float64 weights are then the same numbers and the sums agree to float64 rounding.  The lists
    are built from `incidences`, so this also pins the ownership rule: every corner counted once."""
    X, Y, Z = dims
    C = 4
    rng = np.random.default_rng(3)
    mn, mx = np.zeros(3, np.float32), np.array([X - 1, Y - 1, Z - 1], np.float32)
    M = 4000
    p = (rng.integers(0, 64 * (np.array(dims) - 1) + 1, (M, 3)) / 64.0).astype(np.float32)
    p[:50] = np.round(p[:50])                                # lattice points, box faces included
    g = rng.standard_normal((M, C)).astype(np.float32)
    gd = rng.standard_normal(M).astype(np.float32)
    zeros = np.zeros((M, 3), np.float32)
    O = B.scatter(_sample_recs(M, gd), None, p, zeros, 0.5, mn, mx, g, C, X, Y, Z, by_sample=True)
    grid = torch.zeros((1, C + 1, X, Y, Z), dtype=torch.float64, requires_grad=True)
    ind = ((torch.from_numpy(p).double() - torch.from_numpy(mn).double()) / torch.from_numpy(mx - mn).double()).flip(-1) * 2 - 1
    out = torch.nn.functional.grid_sample(grid, ind[None, None, None], mode='bilinear', align_corners=True)[0, :, 0, 0].t()
    (out * torch.from_numpy(np.concatenate([g, gd[:, None]], 1)).double()).sum().backward()
    want = grid.grad[0].permute(1, 2, 3, 0).reshape(-1, C + 1).numpy()
    assert np.all(np.abs(O.ref - want) <= 1e-12 * O.mag)
    assert np.array_equal(O.mag > 0, want != 0) or np.all(np.abs(want[O.mag == 0]) == 0)
    # the same samples as brick lists
    ijk0, _, _, _ = B.tri_setup(p, mn, mx, X, Y, Z)
    smp, brk = B.incidences(ijk0, X, Y, Z)
    order = np.lexsort((smp, brk))
    nb = int(np.prod(B.n_bricks(X, Y, Z)))
    off = np.concatenate([[0], np.cumsum(np.bincount(brk, minlength=nb))])
    L = B.scatter(_sample_recs(M, gd)[smp[order]], off, p, zeros, 0.5, mn, mx, g, C, X, Y, Z, slice_len=256)
    assert np.array_equal(L.n, O.n) and np.all(np.abs(L.ref - O.ref) <= 1e-12 * O.mag) and np.all(np.abs(L.mag - O.mag) <= 1e-12 * O.mag)
    assert L.S.max() > 1 or off[-1] < 256


def test_incidences_on_hand_built_cases():
    X, Y, Z = 20, 23, 18
    BY, BZ = 3, 3
    bid = lambda x, y, z: (x * BY + y) * BZ + z
    cases = [((3, 4, 5), [bid(0, 0, 0)]),                                           # interior
             ((7, 4, 5), [bid(0, 0, 0), bid(1, 0, 0)]),                             # on a brick face
             ((7, 15, 5), [bid(0, 1, 0), bid(0, 2, 0), bid(1, 1, 0), bid(1, 2, 0)]),  # edge
             ((7, 7, 7), [bid(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)]),  # corner
             ((17, 17, 16), [bid(2, 2, 2)]),                                        # the last, partial brick
             ((19, 22, 17), [bid(2, 2, 2)]),                                        # on xyz_max: upper corners out of range
             ((19, 7, 3), [bid(2, 0, 0), bid(2, 1, 0)]),                            # upper x face and a y brick face
             ((-1, 4, 5), [bid(0, 0, 0)]),                                          # floor corner below the lattice
             ((15, 22, 15), [bid(1, 2, 1), bid(1, 2, 2), bid(2, 2, 1), bid(2, 2, 2)])]
    ijk0 = np.array([c[0] for c in cases], np.int64)
    smp, brk = B.incidences(ijk0, X, Y, Z)
    for i, (_, want) in enumerate(cases):
        assert sorted(brk[smp == i].tolist()) == sorted(want), (cases[i][0], brk[smp == i])
    # against brute force over the corners, on random floor corners
    rng = np.random.default_rng(4)
    ijk0 = rng.integers(-1, 23, (500, 3))
    smp, brk = B.incidences(ijk0, X, Y, Z)
    vb = B.voxel_brick(X, Y, Z).reshape(X, Y, Z)
    for i, (a, b, c) in enumerate(ijk0):
        want = {int(vb[x, y, z]) for x in (a, a + 1) for y in (b, b + 1) for z in (c, c + 1)
                if 0 <= x < X and 0 <= y < Y and 0 <= z < Z}
        assert set(brk[smp == i].tolist()) == want and len(brk[smp == i]) == len(want)


def _step_size(lr, b1, b2, step):
    f = np.float32
    return f(lr) * np.sqrt(f(1) - np.power(f(b2), f(step))) / (f(1) - np.power(f(b1), f(step)))


def test_adam_rule_reproduces_the_masked_adam_fixture_and_the_c_oracle(oracle):
    g = load_golden('masked_adam')
    for tag, masked in (('plain', False), ('masked', True)):
        p = g[f'{tag}_p0'].copy()
        m, v = np.zeros_like(p), np.zeros_like(p)
        for s in range(3):
            B.adam_reference(p, g[f'{tag}_g{s}'], m, v, _step_size(0.1, 0.9, 0.99, s + 1), 0.9, 0.99, 1e-8, masked)
            np.testing.assert_array_equal(p, g[f'{tag}_p{s + 1}'])
        np.testing.assert_array_equal(m, g[f'{tag}_exp_avg'])
    rng = np.random.default_rng(5)
    n = 20000
    p, m, v, gr = (rng.standard_normal(n).astype(np.float32) for _ in range(4))
    v = np.abs(v) * np.float32(0.01)
    gr[rng.uniform(size=n) < 0.3] = 0
    gr[:100] *= np.float32(1e-20); m[::7] = 0; v[::5] = 0
    for masked in (True, False):
        for step in (1, 7):
            a = [x.copy() for x in (p, gr, m, v)]
            b = [x.copy() for x in (p, gr, m, v)]
            oracle.adam_upd(a[0], a[1], a[2], a[3], step, 0.9, 0.99, 0.1, 1e-8, mode=1 if masked else 0)
            B.adam_reference(b[0], b[1], b[2], b[3], _step_size(0.1, 0.9, 0.99, step), 0.9, 0.99, 1e-8, masked)
            for x, y in zip(a, b):
                assert np.array_equal(x.view(np.int32), y.view(np.int32))


def _emulate(O, ins, masked=(1, 1), seed=0, second=False):
    """A float32 stand-in for the kernel: the correctly rounded sums through the float32 Adam rule."""
    X, Y, Z, C = O.shape
    rng = np.random.default_rng(seed)
    g32 = O.ref.astype(np.float32)
    H = B.Hyper(0.1, masked[0], 0.07, masked[1], 0.9, 0.99, 1e-8)
    n = X * Y * Z
    p0 = rng.standard_normal((n, C + 1)).astype(np.float32)
    m0 = (0.1 * rng.standard_normal((n, C + 1))).astype(np.float32) if second else np.zeros((n, C + 1), np.float32)
    v0 = (0.01 * rng.uniform(size=(n, C + 1))).astype(np.float32) if second else np.zeros((n, C + 1), np.float32)
    p1, m1, v1 = p0.copy(), m0.copy(), v0.copy()
    listed = np.broadcast_to(O.listed[:, None], p0.shape)
    for cols, ss, msk in ((slice(0, C), H.ss_k, masked[0]), (slice(C, C + 1), H.ss_d, masked[1])):
        a = [x[:, cols].copy() for x in (p1, m1, v1)]
        B.adam_reference(a[0], g32[:, cols], a[1], a[2], ss, 0.9, 0.99, 1e-8, bool(msk))
        for x, y in zip((p1, m1, v1), a):
            x[:, cols] = np.where(listed[:, cols], y, x[:, cols])

    def grids(p, m, v):          # voxel-major -> the parameters' own shapes
        k = lambda a: np.moveaxis(a[:, :C].reshape(X, Y, Z, C), -1, 0)[None]
        d = lambda a: a[:, C].reshape(1, 1, X, Y, Z)
        return [k(p), k(m), k(v), d(p), d(m), d(v)]
    return H, grids(p0, m0, v0), [p1, m1, v1], grids, g32


@pytest.mark.parametrize('masked', [(1, 1), (0, 0), (1, 0)])
def test_the_checks_pass_a_float32_emulation_and_fail_value_only_faults(masked):
    ins, counts = B.synthetic_case('shifted', 12)
    O = B.scatter(**ins, slice_len=B.SYN_SLICE)
    X, Y, Z, C = O.shape
    H, before, (p1, m1, v1), grids, g32 = _emulate(O, ins, masked, second=True)
    k0 = np.moveaxis(g32[:, :C].reshape(X, Y, Z, C), -1, 0)[None]
    assert B.check_dense(O, k0, g32[:, C]) <= 1.0
    st = B.check_adam(O, before, grids(p1, m1, v1), H)
    assert st['undetermined'] == 0 and st['nonzero'] > 10000
    heavy = np.nonzero((O.n > 0) & (O.mag[:, 1] > 0))[0]
    # a dropped corner: one term of one voxel missing from the dense gradient
    bad = g32.copy()
    vox = heavy[np.argmax(O.n[heavy])]
    bad[vox, 1] -= np.float32(O.mag[vox, 1] / O.n[vox])
    with pytest.raises(AssertionError, match='outside gamma'):
        B.check_dense(O, np.moveaxis(bad[:, :C].reshape(X, Y, Z, C), -1, 0)[None], bad[:, C])
    # a non-zero where nothing contributes
    bad = g32.copy()
    bad[np.nonzero(O.mag[:, 0] == 0)[0][0], 0] = 1e-30
    with pytest.raises(AssertionError, match='non-zero gradient'):
        B.check_dense(O, np.moveaxis(bad[:, :C].reshape(X, Y, Z, C), -1, 0)[None], bad[:, C])
    # m.y of one voxel not updated while v is (the recorded fault)
    m_bad = m1.copy()
    m_bad[heavy[3], 1] = _emulate(O, ins, masked, second=True)[1][1].reshape(C, -1)[1, heavy[3]]
    with pytest.raises(AssertionError, match='m not'):
        B.check_adam(O, before, grids(p1, m_bad, v1), H)
    # p stepped from another first moment than the one stored
    p_bad = p1.copy()
    p_bad[heavy[5], 2] += np.float32(3e-6)
    with pytest.raises(AssertionError, match='p not'):
        B.check_adam(O, before, grids(p_bad, m1, v1), H)
    # v from another gradient
    v_bad = v1.copy()
    v_bad[heavy[7], C] *= np.float32(1.001)
    with pytest.raises(AssertionError, match='v not'):
        B.check_adam(O, before, grids(p1, m1, v_bad), H)
    if masked[0]:
        # an element without any contribution that moved (a float4-wide masked test lets its neighbours through)
        p_bad = p1.copy()
        idle = np.nonzero(O.mag[:, 0] == 0)[0][0]
        p_bad[idle, 0] = np.nextafter(p_bad[idle, 0], np.float32(9))
        with pytest.raises(AssertionError, match='changed where no gradient'):
            B.check_adam(O, before, grids(p_bad, m1, v1), H)


@pytest.mark.parametrize('family', B.SYN_FAMILIES)
def test_undetermined_share_of_every_synthetic_input_the_gpu_tests_launch(family):
    """Measured on the CPU: of the elements with a contribution, the share whose float64 sum is within the gradient bound of
    zero (their masked-Adam branch is not determined).  The all-on-one-voxel brick is part of every case."""
    for C in (3, 4, 9, 12):
        for sl in B.SYN_SLICES:
            A, cA = B.synthetic_case(family, C, 'A', sl)
            Bq, cB = B.synthetic_case(family, C, 'B', sl)
            OA, OB = B.scatter(**A, slice_len=sl), B.scatter(**Bq, slice_len=sl)
            for O in (OA, OB, OA + OB, B.scatter(**A, slice_len=0)):
                share = B.undetermined_share(O)
                print(family, C, sl, 'share', share, 'max n', int(O.n.max()))
                assert share <= B.MAX_UNDETERMINED
            assert OA.n.max() >= 512 and cA.max() == 3 * sl + 7 and ((cA > 0) & (cB == 0)).any() and ((cB > 0) & (cA == 0)).any()
            assert OA.S.max() == 4 and OB.S.max() == 3
