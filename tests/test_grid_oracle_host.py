"""CPU: tests/grid_oracle.py and tests/grid_cases.py held to what they restate, before any GPU test relies on them.

  * the view-weight positions against the C oracle's slab test and the reference's sampler expression, bit for bit, and
    the view sums against float64 autograd of torch's grid_sample of ones;
  * the three bounds in both directions: float32 emulations of the kernels in three summation orders stay inside with no
    element excluded, and value-only faults of the kind the suite exists for fall outside;
  * every edge-table row: the floor corner and the in-range mask it claims are what the float32 setup finds, on the
    C oracle too for the lattices with a unit axis;
  * the undetermined share of every input the GPU count test launches, from the oracle alone;
  * the overflow certificate of the input the GPU overflow test launches.
"""
import numpy as np
import pytest
import torch

import brick_oracle as B
import grid_cases as K
import grid_oracle as G
from conftest import load_golden

F = np.float32


# ------------------------------------------------------------------------------------------ emulations
def _sum32(idx, terms, n, order='serial', group=None):
    """float32 sums of `terms` by `idx` in a stated order (np.add.at adds unbuffered, in index order, in float32)"""
    idx, terms = np.asarray(idx, np.int64), np.asarray(terms, np.float32)
    acc = np.zeros(n, np.float32)
    if order == 'serial':
        np.add.at(acc, idx, terms)
    elif order == 'reversed':
        np.add.at(acc, idx[::-1], terms[::-1])
    else:                                                   # 'table': sums per (group, idx) first, then those into memory
        key = np.asarray(group, np.int64) * n + idx
        uniq, inv = np.unique(key, return_inverse=True)
        table = np.zeros(uniq.shape[0], np.float32)
        np.add.at(table, inv, terms)
        np.add.at(acc, uniq % n, table)
    return acc


ORDERS = ('serial', 'reversed', 'table')


def _scatter_emulation(xyz, gout, dims, order, prefill=None, fault=None):
    """[C, X, Y, Z] float32: each product rounded once, then float32 additions in `order` (groups of 64 samples)"""
    X, Y, Z = dims
    C = gout.shape[1]
    ijk0, w, inb, vox = B.tri_setup(xyz, K.MN, K.MX, X, Y, Z)
    w = w.copy()
    if fault == 'corner dropped on a face':
        inb = inb & ~((ijk0[:, 0] == X - 1)[:, None] & (np.arange(8) == 0)[None, :])
    if fault == 'weights of two corners swapped':
        w[:, [1, 2]] = w[:, [2, 1]]
    e, q = np.nonzero(inb)
    out = np.zeros((C, X * Y * Z), np.float32)
    for c in range(C):
        terms = w[e, q] * gout[e, c]
        keep = np.ones(e.shape[0], bool)
        if fault == 'last thread of the last block idle' and c == C - 1:
            keep = e != xyz.shape[0] - 1
        acc = _sum32(vox[e, q][keep], terms[keep], X * Y * Z, order, group=(e // 64)[keep])
        if prefill is not None:
            pre = prefill[c].reshape(-1)
            acc = (pre + acc).astype(np.float32)
        out[c] = acc
    return out.reshape(C, X, Y, Z)


# ------------------------------------------------------------------------------------------ edge rows
@pytest.mark.parametrize('dims', K.LATTICES)
def test_every_edge_row_lands_where_it_says(dims, oracle):
    names = [n for n, _ in K.edge_rows(dims)]
    assert {'nodes', 'faces', 'out1', 'beyond', 'corners', 'pile_inside', 'pile_face'} <= set(names)
    assert ('out3' in names) == (min(dims) > 1)
    for name, g in K.edge_rows(dims):
        xyz, i0 = K.points(g, dims)
        ijk0, w, inb, _ = B.tri_setup(xyz, K.MN, K.MX, *dims)
        assert np.array_equal(ijk0, i0), name
        assert np.array_equal(inb, K.in_range(i0, dims)), name
        if name in ('nodes', 'corners', 'faces'):
            on_node = g == np.round(g)
            full = on_node.all(1)
            assert np.all(np.isin(w[full], (0.0, 1.0))) and np.all(w[full].sum(1) == 1), name
            assert np.all((w == 0).sum(1) >= 4), name           # a node on one axis zeroes the four corners beyond it
        if name == 'beyond':
            assert not inb.any()
        if name.startswith('out'):
            k = int(name[3])
            free = sum(s > 1 for s in dims)
            assert np.all(inb.sum(1) == 2 ** (free - k)), name
        if name.startswith('pile'):
            assert xyz.shape[0] == K.PILE and np.all(xyz == xyz[0]) and inb[0].sum() == (2 ** sum(s > 1 for s in dims)) // (1 + (name == 'pile_face'))
    # the restated setup on these rows is the C oracle's (tests/test_brick_oracle_host.py pins it on cubic-ish lattices; the
    # unit axes and the rows beyond the faces are added here): a single contribution involves no summation
    X, Y, Z = dims
    rng = np.random.default_rng(1)
    for name, g in K.edge_rows(dims):
        xyz = K.points(g[:12], dims)[0]
        for p in xyz:
            go = rng.standard_normal((1, 2)).astype(F)
            want = oracle.grid_sample_bwd(go, (2, X, Y, Z), p[None], K.MN, K.MX)
            O = G.scatter_sums(p[None], go, K.MN, K.MX, dims)
            got = np.moveaxis(O.ref[:, :2].astype(F).reshape(X, Y, Z, 2), -1, 0)
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (name, p)


def test_sample_counts_cross_the_block_edge():
    assert K.SAMPLE_COUNTS == [1, 255, 256, 257, 5003] and K.CHANNELS == [1, 3, 4, 9, 12]
    for C in (3, 9, 12):
        tails = {(M * C) % 256 for M in K.SAMPLE_COUNTS}
        assert 0 in tails and len(tails) >= 4                       # M * C both on and off the 256-thread edge
    for dims in K.LATTICES:
        assert int(np.prod(dims)) <= 2300
        for M in K.SAMPLE_COUNTS:
            p = K.random_points(dims, M, 1)
            _, _, inb, _ = B.tri_setup(p, K.MN, K.MX, *dims)
            assert p.shape == (M, 3)
            if M > 200:
                full = 2 ** sum(s > 1 for s in dims)                  # a unit axis never has its upper corner in range
                assert (inb.sum(1) == full).any() and (inb.sum(1) < full).any() and (inb.sum(1) == 0).any()


# ------------------------------------------------------------------------------------------ scatter: the bound both ways
@pytest.mark.parametrize('dims', [(5, 7, 9), (1, 5, 6)])
def test_scatter_bound_holds_in_three_orders_and_catches_faults(dims):
    C = 3
    xyz = np.concatenate([K.edge_points(dims), K.random_points(dims, 257, 3)])
    gout = K.grad_out(xyz.shape[0], C, 5)
    O = G.scatter_sums(xyz, gout, K.MN, K.MX, dims)
    assert O.n.max() >= K.PILE
    for order in ORDERS:
        r = G.check_scatter(O, _scatter_emulation(xyz, gout, dims, order), order)
        assert 0 < r <= 1
    pre = K.grid_values(C, dims, 9)
    Op = G.scatter_sums(xyz, gout, K.MN, K.MX, dims, prefill=pre)
    for order in ORDERS:
        assert G.check_scatter(Op, _scatter_emulation(xyz, gout, dims, order, prefill=pre), order) <= 1
    faults = ['weights of two corners swapped', 'last thread of the last block idle']
    if dims[0] > 1:
        faults.append('corner dropped on a face')
    for fault in faults:
        with pytest.raises(AssertionError):
            G.check_scatter(O, _scatter_emulation(xyz, gout, dims, 'serial', fault=fault), fault)
    with pytest.raises(AssertionError):                       # accumulate means accumulate: the pre-fill must survive
        G.check_scatter(Op, _scatter_emulation(xyz, gout, dims, 'serial'), 'pre-fill overwritten')
    bad = _scatter_emulation(xyz, gout, dims, 'serial')
    untouched = np.argwhere(np.moveaxis(O.mag[:, :C].reshape(*dims, C), -1, 0) == 0)
    if untouched.size:
        bad[tuple(untouched[0])] = 1e-30                     # a write where nothing contributes, however small
        with pytest.raises(AssertionError, match='no term contributes'):
            G.check_scatter(O, bad, 'stray write')


# ------------------------------------------------------------------------------------------ view weights
def test_view_positions_follow_the_c_oracle_and_the_reference_expression(oracle):
    g = load_golden('voxel_count_views')
    ws = tuple(int(v) for v in g['world_size'])
    stepsize, vs = float(g['stepsize']), F(g['voxel_size'])
    S = int(np.linalg.norm(np.array(ws) + 1) / stepsize) + 1
    step = F(stepsize) * vs
    near, far = float(g['near']), float(g['far'])
    ro, rd = g['rays_o'].reshape(-1, 3), g['rays_d'].reshape(-1, 3)
    # zero components, a miss and a start inside ride along with the fixture's rays
    o2, d2 = K.view_rays(16, 3)
    ro, rd = np.concatenate([ro, o2]), np.concatenate([rd, d2])
    pos = G.view_positions(ro, rd, g['xyz_min'], g['xyz_max'], near, far, step, S)
    # the slab test: ora_infer_t_minmax, recovered from sample 0 (t = t_min + 0 / norm = t_min) ...
    t_min, _ = oracle.infer_t_minmax(ro, rd, g['xyz_min'], g['xyz_max'], near, far)
    assert np.array_equal(pos[:, 0].view(np.int32), (ro + rd * t_min[:, None]).astype(F).view(np.int32))
    # ... and the sampler the way tests/test_oracle_golden.py states the reference's (lib/dvgo.py:286-288)
    steps = (step * np.arange(S, dtype=F))[None]
    interpx = t_min[:, None] + steps / np.linalg.norm(rd, axis=-1, keepdims=True).astype(F)
    ref_pts = (ro[:, None] + rd[:, None] * interpx[..., None]).astype(F)
    sq = rd * rd
    same_norm = np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2]) == np.linalg.norm(rd, axis=-1).astype(F)
    assert same_norm.mean() > 0.5                           # numpy's norm may sum in another order: compare where it agrees
    assert np.array_equal(pos[same_norm].view(np.int32), ref_pts[same_norm].view(np.int32))
    # sums: float64 autograd of F.grid_sample of ones at those (float32) positions
    V = G.view_sums(pos, g['xyz_min'], g['xyz_max'], ws)
    ones = torch.ones((1, 1, *ws), dtype=torch.float64, requires_grad=True)
    p64 = torch.from_numpy(pos.reshape(-1, 3))
    mn, mx = torch.from_numpy(g['xyz_min']), torch.from_numpy(g['xyz_max'])
    u32 = (p64 - mn) / (mx - mn)                             # float32, as the setup: the weights' input is then the same number
    ind = (u32.flip(-1) * 2 - 1)
    out = torch.nn.functional.grid_sample(ones, ind.double()[None, None, None], mode='bilinear', align_corners=True)
    out.sum().backward()
    want = ones.grad.reshape(-1).numpy()
    # torch unnormalises in float64 from the float32 c; the restated setup rounds g and the weights to float32
    # (3 roundings on g relative to the lattice size, 2 per weight product): compare to the float32 setup's own accuracy
    tol = 16 * max(ws) * B.U * np.maximum(V.n, 1)
    assert np.all(np.abs(V.ref - want) <= tol)
    assert np.all((want != 0) <= (V.n > 0))


def test_view_sums_equal_float64_autograd_where_the_setup_is_exact():
    """Box and positions chosen so that the float32 setup is exact (line_case's lattice, positions on a 1/64 voxel grid):
    torch's float64 weights are then the same numbers and the sums agree to 1e-12 relative."""
    dims = K.LINE_DIMS
    rng = np.random.default_rng(4)
    size1 = np.array(dims) - 1
    gq = rng.integers(-64, 64 * (size1 + 1) + 1, (6000, 3)) / 64.0
    pos = (K.MN + gq / size1 * (K.MX - K.MN).astype(np.float64)).astype(F)
    _, w, inb, _ = B.tri_setup(pos, K.MN, K.MX, *dims)
    V = G.view_sums(pos, K.MN, K.MX, dims)
    ones = torch.ones((1, 1, *dims), dtype=torch.float64, requires_grad=True)
    ind = ((torch.from_numpy(pos).double() - torch.from_numpy(K.MN).double()) / torch.from_numpy(K.MX - K.MN).double()).flip(-1) * 2 - 1
    torch.nn.functional.grid_sample(ones, ind[None, None, None], mode='bilinear', align_corners=True).sum().backward()
    want = ones.grad.reshape(-1).numpy()
    assert np.all(np.abs(V.ref - want) <= 1e-12 * V.mag) and V.n.max() > 8
    assert np.array_equal(V.mag, V.ref)                      # weights are never negative


def _view_emulation(case, order, fault=None):
    dims = case['dims']
    pos = G.view_positions(case['rays_o'], case['rays_d'], K.MN, K.MX, case['near'], case['far'], case['step'], case['n_samples'])
    S = case['n_samples']
    e, v, w = G.view_terms(pos, K.MN, K.MX, dims)
    ray, k = e // S, e % S
    table = ray * ((S + 63) // 64) + k // 64                 # one table per wavefront pass
    keep = np.ones(e.shape[0], bool)
    nvox = int(np.prod(dims))
    if fault == 'weight lost on table overflow':
        keep[int(np.argmax(w))] = False
    if fault == 'sample 64 skipped at the chunk boundary':
        keep = k != 64
    acc = _sum32(v[keep], w[keep], nvox, order, group=table[keep])
    if fault == 'table not cleared between chunks':          # chunk 0's entries go out again with chunk 1
        again = (k // 64 == 0) & (S > 64)
        acc = (acc + _sum32(v[again], w[again], nvox, 'serial')).astype(F)
    return G.view_sums(pos, K.MN, K.MX, dims), acc


@pytest.mark.parametrize('case', ['view', 'contended', 'overflow', 'line'])
def test_view_bound_holds_in_three_orders_and_catches_faults(case):
    c = {'view': lambda: K.view_case(256, 200), 'contended': K.contended_case, 'overflow': K.overflow_case, 'line': K.line_case}[case]()
    for order in ORDERS:
        V, acc = _view_emulation(c, order)
        r = G.check_view(V, acc, order)
        assert r <= 1 and V.n.max() > 1
    if case == 'line':
        assert set(np.unique(V.ref)) == {0.0, 5.0} and np.array_equal(acc.astype(np.float64), V.ref)
        assert int((V.ref == 5).sum()) == 17
    if case == 'contended':
        assert (V.n > 0).sum() == 8 and V.n.min() >= 100
    faults = ['weight lost on table overflow']
    if c['n_samples'] > 64:
        faults.append('table not cleared between chunks')
    if c['n_samples'] > 64 and case != 'line':               # the line's sample 64 lies beyond the box
        faults.append('sample 64 skipped at the chunk boundary')
    for fault in faults:
        V, acc = _view_emulation(c, 'table', fault)
        with pytest.raises(AssertionError):
            G.check_view(V, acc, fault)
    V, acc = _view_emulation(c, 'serial')
    if (V.n == 0).any():
        acc[int(np.argmax(V.n == 0))] = 1e-30
        with pytest.raises(AssertionError, match='no sample reaches'):
            G.check_view(V, acc, 'stray write')


def test_view_cases_are_what_they_say():
    for n_rays in K.VIEW_RAYS:
        for S in K.VIEW_SAMPLES:
            c = K.view_case(n_rays, S)
            pos = G.view_positions(c['rays_o'], c['rays_d'], K.MN, K.MX, c['near'], c['far'], c['step'], S)
            assert pos.shape == (n_rays, S, 3) and np.all(np.isfinite(pos))
    c = K.view_case(256, 200)
    assert (256 * 64) % 256 == 0 and (5 * 64) % 256 != 0            # the last block of 5 rays is partly filled
    o, d = c['rays_o'], c['rays_d']
    assert (d[0] == 0).sum() == 2 and (d[1] == 0).sum() == 1 and (d[4] == 0).sum() == 2
    pos = G.view_positions(o, d, K.MN, K.MX, c['near'], c['far'], c['step'], 200)
    hits = [G.view_sums(pos[i], K.MN, K.MX, c['dims']).n.sum() for i in range(5)]
    assert hits[0] > 0 and hits[1] > 0 and hits[3] > 0 and hits[2] == 0 and hits[4] == 0      # ray 2 misses, ray 4 points away
    assert np.all((o[3] > K.MN) & (o[3] < K.MX))                                              # ray 3 starts inside


def test_count_rule_and_the_undetermined_share_of_the_count_case():
    V = G.ViewSums(np.array([0.0, 0.5, 1.0, 1.0 + 1e-9, 1.0 - 1e-9, 1.0 + 1e-3, 37.5]), np.array([0.0, 0.5, 1.0, 1.0, 1.0, 1.001, 37.5]),
                   np.array([0, 3, 4, 4, 4, 4, 90]), (7, 1, 1))
    c, n, u = G.count_rule(V)
    assert c.tolist() == [False, False, False, False, False, True, True]
    assert n.tolist() == [True, True, False, False, False, False, False]
    assert u.tolist() == [False, False, True, True, True, False, False]
    case = K.count_case()
    views = []
    for v in range(K.COUNT_VIEWS):
        pos = G.view_positions(case['rays_o'][v], case['rays_d'][v], K.COUNT_MIN, K.COUNT_MAX, K.COUNT_NEAR, K.COUNT_FAR, case['step'],
                               case['n_samples'])
        V = G.view_sums(pos, K.COUNT_MIN, K.COUNT_MAX, K.COUNT_DIMS)
        views.append(V)
        assert G.undetermined_share(V) <= 0.01
        counted = G.count_rule(V)[0]
        assert counted.sum() > 500 and (V.ref > 0).sum() > counted.sum() + 200      # both sides of the threshold are populated
    for c in (K.view_case(256, 200), K.view_case(5, 65)):      # the two views of the commit-in-between test
        pos = G.view_positions(c['rays_o'], c['rays_d'], K.MN, K.MX, c['near'], c['far'], c['step'], c['n_samples'])
        assert G.undetermined_share(G.view_sums(pos, K.MN, K.MX, c['dims'])) <= 0.01
    exact = sum(G.count_rule(V)[0].astype(np.float64) for V in views)
    assert exact.max() == 3
    G.check_counts(views, exact)
    wrong = exact.copy()
    wrong[int(np.argmax(exact == 3))] = 2                    # a view that lost a determined voxel
    with pytest.raises(AssertionError):
        G.check_counts(views, wrong)


# ------------------------------------------------------------------------------------------ the table's hash
def test_hash_restatement_and_the_overflow_certificate_of_the_chosen_input():
    assert G.hash_home([0, 1, 2]).tolist() == [0, (2654435761 % 2 ** 32) >> 23, ((2 * 2654435761) % 2 ** 32) >> 23]
    assert G.hash_home(np.arange(3000)).max() < 512
    # 17 keys with one home: the 17th finds no slot in 16 probes; a key met again finds its own slot
    homes = G.hash_home(np.arange(200000))
    same = np.nonzero(homes == homes[5])[0][:17]
    assert G.place(same).tolist() == [True] * 16 + [False]
    assert G.place(np.concatenate([same[:16], same[:16]])).all()
    assert G.overflow_certificate(same[:16]) is None and G.overflow_certificate(same) == (int(homes[5]), 16, 17)
    assert G.overflow_certificate(np.arange(513)) == (0, 512, 513)
    keys = K.overflow_keys()
    assert keys.shape[0] == 512 and np.unique(keys).shape[0] == 512          # eight keys of its own for every sample
    a, L, inside = G.overflow_certificate(keys)
    h = np.unique(keys)
    rel = (G.hash_home(h) - a) % 512
    assert inside == int((rel <= L - 16).sum()) and inside > L               # whole windows inside [a, a + L), more keys than slots
    for order in (keys, keys[::-1], np.random.default_rng(0).permutation(keys)):
        assert (~G.place(order)).sum() >= inside - L
    c = K.overflow_case()
    assert float(c['step']) / ((K.MX[0] - K.MN[0]) / (c['dims'][0] - 1)) >= 2 and int(np.prod(c['dims'])) <= 2200


# ------------------------------------------------------------------------------------------ segment sum
def _segment_emulation(case, order, fault=None):
    src, index, out0 = case['src'], case['index'], case['out0']
    N, C = out0.shape
    M = src.shape[0]
    rows = np.arange(M)
    keep = np.ones(M, bool)
    if fault == 'tail missed at lane 63':                    # a segment that ends on lane 63: its last wave part is lost
        ends = np.nonzero((np.diff(index, append=N) != 0) & (rows % 64 == 63))[0]
        keep = ~((index == index[ends[0]]) & (rows // 64 == ends[0] // 64))
    if fault == 'rows past the last full wave dropped':
        keep = rows < (M // 64) * 64
    out = np.empty((N, C), np.float32)
    for c in range(C):
        acc = _sum32(index[keep], src[keep, c], N, order, group=(rows // 64)[keep])
        out[:, c] = acc if fault == 'initial value overwritten' else (out0[:, c] + acc).astype(F)
    return out


@pytest.mark.parametrize('C', [1, 3, 4])
def test_segment_bound_holds_in_three_orders_and_catches_faults(C):
    case = K.segment_case(C)
    lens, index = case['lens'], case['index']
    M = index.shape[0]
    ends = np.cumsum(lens)[lens > 0] - 1
    assert M % 64 != 0 and {1, 63, 64, 65, 256, 257, 5003} <= set(lens.tolist())
    assert lens[0] == 0 and lens[-1] == 0 and (lens[1:-1] == 0).any()
    assert (ends % 64 == 63).sum() >= 3 and (ends % 256 == 255).sum() >= 2
    S = G.segment_sums(case['src'], index, case['out0'])
    assert (S.mag > 1e4 * np.abs(S.ref)).any()               # cancellation: the bound is relative to mag, not to |ref|
    for order in ORDERS:
        r = G.check_segment(S, _segment_emulation(case, order), case['out0'], order)
        assert 0 < r <= 1
    for fault in ('tail missed at lane 63', 'rows past the last full wave dropped', 'initial value overwritten'):
        with pytest.raises(AssertionError):
            G.check_segment(S, _segment_emulation(case, 'table', fault), case['out0'], fault)
    moved = _segment_emulation(case, 'serial')
    moved[0] = np.nextafter(moved[0], F(9))                  # an empty segment must keep its bits
    with pytest.raises(AssertionError, match='without rows'):
        G.check_segment(S, moved, case['out0'])
