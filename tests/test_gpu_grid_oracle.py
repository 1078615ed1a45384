"""GPU: the op-by-op trilinear family and the per-ray sum held elementwise to tests/grid_oracle.py.

  dvgo_grid_sample_fwd          bit-equal to the C oracle on every edge row, lattice, channel count, layout and dispatch
                                branch (vector / generic; misaligned grid or out; a strided sub-box of a larger grid)
  dvgo_grid_sample_bwd          `check_dense(atomic=True)` elementwise, exact zeros where nothing contributes: through
                                ops.grid_sample(...).backward and through the ABI into a pre-filled grad_grid
  dvgo_view_weight_accumulate   `acc` before any commit against the float64 sums of the restated positions
  dvgo_view_count_commit        exact counts and an exactly cleared accumulator on hand-made values
  DirectVoxGO.voxel_count_views every voxel the oracle can decide is exact
  dvgo_segment_sum              any-order bound with `out`'s initial value as a term, empty segments bit for bit

tests/test_grid_oracle_host.py holds the oracle and the inputs to their own references on the CPU.  The worst err / bound
per kernel is printed when the module finishes (pytest -s); it is information, never a threshold.
"""
import numpy as np
import pytest
import torch

import grid_cases as K
import grid_oracle as G

pytestmark = pytest.mark.gpu

WORST = {}


def _note(kernel, r):
    WORST[kernel] = max(WORST.get(kernel, 0.0), float(r))


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print(f'\nworst err / bound  {k}: {WORST[k]:.4f}', end='')
    print()


@pytest.fixture(scope='module')
def ops():
    from directvoxgo_amd import ops
    return ops


@pytest.fixture(scope='module')
def L():
    from directvoxgo_amd import _lib
    return _lib


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def channels_last(t):
    """[1, C, X, Y, Z] -> the same values with strides (., 1, Y Z C, Z C, C)"""
    _, C, X, Y, Z = t.shape                    # strides stated outright: .contiguous() keeps whatever a size-1 axis had
    out = torch.empty_strided(t.shape, (X * Y * Z * C, 1, Y * Z * C, Z * C, C), dtype=t.dtype, device=t.device)
    return out.copy_(t)


def in_layout(grid_np, layout):
    g = cu(grid_np)[None]
    g = channels_last(g) if layout == 'cl' else g.contiguous()
    C = g.shape[1]
    if layout == 'cl':
        assert g.stride(1) == 1 and g.stride(4) == C
    return g


def abi_fwd(L, grid, xyz, mn, mx, out):
    _, C, X, Y, Z = grid.shape
    _, sC, sX, sY, sZ = grid.stride()
    L.call('dvgo_grid_sample_fwd', grid, C, X, Y, Z, sC, sX, sY, sZ, xyz, mn, mx, xyz.shape[0], out, L.stream_of(xyz))
    return out


def abi_bwd(L, grad_out, xyz, mn, mx, grad_grid):
    _, C, X, Y, Z = grad_grid.shape
    _, sC, sX, sY, sZ = grad_grid.stride()
    L.call('dvgo_grid_sample_bwd', grad_out, C, X, Y, Z, sC, sX, sY, sZ, xyz, mn, mx, xyz.shape[0], grad_grid, L.stream_of(xyz))
    return grad_grid


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.int32), np.asarray(b, np.float32).view(np.int32))


BOX = None


def box():
    global BOX
    if BOX is None:
        BOX = (cu(K.MN), cu(K.MX))
    return BOX


def _run_all_paths(ops, L, oracle, dims, C, xyz, seed):
    """forward and backward of one point list in both layouts, through autograd and through the ABI"""
    mn, mx = box()
    M = xyz.shape[0]
    grid = K.grid_values(C, dims, seed)
    gout = K.grad_out(M, C, seed + 1)
    pre = K.grid_values(C, dims, seed + 2)
    want = G.gather(oracle, grid, xyz, K.MN, K.MX)
    O = G.scatter_sums(xyz, gout, K.MN, K.MX, dims)
    Op = G.scatter_sums(xyz, gout, K.MN, K.MX, dims, prefill=pre)
    x, go = cu(xyz), cu(gout)
    for layout in ('cf', 'cl'):
        g = in_layout(grid, layout).requires_grad_()
        out = ops.grid_sample(g, x, mn, mx)
        assert same_bits(host(out).reshape(M, C), want), (layout, 'forward')
        (gg,) = torch.autograd.grad(out.reshape(M, C), g, go)
        assert gg.stride() == g.stride()
        _note('grid_sample_bwd ' + ('(sample, channel) kernel' if layout == 'cl' and C > 1 else 'per-sample kernel'),
              G.check_scatter(O, host(gg)[0], f'{layout} backward'))
        out2 = abi_fwd(L, g.detach(), x, mn, mx, torch.full((M, C), 7.0, device='cuda'))
        assert same_bits(host(out2), want), (layout, 'forward through the ABI')
        acc = in_layout(pre, layout)
        abi_bwd(L, go, x, mn, mx, acc)
        _note('grid_sample_bwd into a pre-filled grad_grid', G.check_scatter(Op, host(acc)[0], f'{layout} backward, pre-filled'))


# ------------------------------------------------------------------------------------------ grid_sample
@pytest.mark.parametrize('C', K.CHANNELS)
@pytest.mark.parametrize('dims', K.LATTICES)
def test_grid_sample_edge_rows(ops, L, oracle, dims, C):
    _run_all_paths(ops, L, oracle, dims, C, K.edge_points(dims), 100 + C)


@pytest.mark.parametrize('C', K.CHANNELS)
@pytest.mark.parametrize('M', K.SAMPLE_COUNTS)
def test_grid_sample_sample_counts(ops, L, oracle, M, C):
    dims = (5, 7, 9) if C in (3, 9, 12) else (17, 4, 33)
    _run_all_paths(ops, L, oracle, dims, C, K.random_points(dims, M, 10 * M + C), 200 + C)


@pytest.mark.parametrize('C', [4, 12])
@pytest.mark.parametrize('which', ['grid', 'out', 'both'])
def test_grid_sample_vector_path_declines_misaligned_buffers(L, oracle, which, C):
    """A channels-last grid (and an `out`) whose base is 4 bytes past a 16-byte boundary: a slice of a flat buffer."""
    dims = (5, 7, 9)
    X, Y, Z = dims
    mn, mx = box()
    xyz = np.concatenate([K.edge_points(dims)[:80], K.random_points(dims, 257, C)])
    M = xyz.shape[0]
    grid = K.grid_values(C, dims, 300 + C)
    want = G.gather(oracle, grid, xyz, K.MN, K.MX)
    off_g, off_o = int(which in ('grid', 'both')), int(which in ('out', 'both'))
    flat = torch.zeros(X * Y * Z * C + 4, device='cuda')
    g = flat[off_g:off_g + X * Y * Z * C].view(1, X, Y, Z, C).permute(0, 4, 1, 2, 3)
    g.copy_(cu(grid)[None])
    oflat = torch.full((M * C + 4,), 7.0, device='cuda')
    out = oflat[off_o:off_o + M * C].view(M, C)
    assert g.data_ptr() % 16 == 4 * off_g and out.data_ptr() % 16 == 4 * off_o and g.stride(1) == 1
    abi_fwd(L, g, cu(xyz), mn, mx, out)
    assert same_bits(host(out), want)
    assert torch.all(oflat[:off_o] == 7.0) and torch.all(oflat[off_o + M * C:] == 7.0)
    gout = K.grad_out(M, C, 301)
    gflat = torch.zeros_like(flat)
    gg = gflat[off_g:off_g + X * Y * Z * C].view(1, X, Y, Z, C).permute(0, 4, 1, 2, 3)
    abi_bwd(L, cu(gout), cu(xyz), mn, mx, gg)
    _note('grid_sample_bwd (sample, channel) kernel', G.check_scatter(G.scatter_sums(xyz, gout, K.MN, K.MX, dims), host(gg)[0], 'misaligned'))
    assert torch.all(gflat[:off_g] == 0) and torch.all(gflat[off_g + X * Y * Z * C:] == 0)


@pytest.mark.parametrize('C', [1, 3, 4, 12])
@pytest.mark.parametrize('layout', ['cf', 'cl'])
def test_grid_sample_on_a_sub_box_of_a_larger_grid(L, oracle, layout, C):
    """Non-dense strides in both directions; every element of the larger gradient buffer outside the view stays exactly 0."""
    dims = (5, 7, 9)
    X, Y, Z = dims
    mn, mx = box()
    big_np = K.grid_values(C, (X + 3, Y + 2, Z + 4), 400 + C)
    big = in_layout(big_np, layout)
    sub = (slice(None), slice(None), slice(1, 1 + X), slice(2, 2 + Y), slice(1, 1 + Z))
    view = big[sub]
    assert not view.is_contiguous() and view.stride() == big.stride()
    xyz = np.concatenate([K.edge_points(dims)[:80], K.random_points(dims, 257, 40 + C)])
    M = xyz.shape[0]
    grid = np.ascontiguousarray(big_np[:, 1:1 + X, 2:2 + Y, 1:1 + Z])
    out = abi_fwd(L, view, cu(xyz), mn, mx, torch.empty((M, C), device='cuda'))
    assert same_bits(host(out), G.gather(oracle, grid, xyz, K.MN, K.MX))
    gout = K.grad_out(M, C, 401)
    gbig = torch.zeros_like(big)
    assert gbig.stride() == big.stride()
    abi_bwd(L, cu(gout), cu(xyz), mn, mx, gbig[sub])
    r = G.check_scatter(G.scatter_sums(xyz, gout, K.MN, K.MX, dims), host(gbig[sub])[0], f'sub-box {layout}')
    _note('grid_sample_bwd ' + ('(sample, channel) kernel' if layout == 'cl' and C > 1 else 'per-sample kernel'), r)
    outside = gbig.clone()
    outside[sub] = 0
    assert int(torch.count_nonzero(outside)) == 0


# ------------------------------------------------------------------------------------------ view weights
def accumulate(L, case, acc=None):
    dims = case['dims']
    o, d = cu(case['rays_o']), cu(case['rays_d'])
    if acc is None:
        acc = torch.zeros(int(np.prod(dims)), device='cuda')
    L.call('dvgo_view_weight_accumulate', o, d, o.shape[0], L.f3(K.MN), L.f3(K.MX), float(case['near']), float(case['far']),
           float(case['step']), int(case['n_samples']), *dims, acc, L.stream_of(o))
    return acc


def sums_of(case):
    pos = G.view_positions(case['rays_o'], case['rays_d'], K.MN, K.MX, case['near'], case['far'], case['step'], case['n_samples'])
    return G.view_sums(pos, K.MN, K.MX, case['dims'])


@pytest.mark.parametrize('n_samples', K.VIEW_SAMPLES)
@pytest.mark.parametrize('n_rays', K.VIEW_RAYS)
def test_view_weights(L, n_rays, n_samples):
    case = K.view_case(n_rays, n_samples)
    _note('view_weight', G.check_view(sums_of(case), host(accumulate(L, case)), f'{n_rays} rays, {n_samples} samples'))


def test_view_weights_along_a_lattice_line_are_exact_integers(L):
    case = K.line_case()
    V = sums_of(case)
    acc = host(accumulate(L, case))
    _note('view_weight', G.check_view(V, acc, 'lattice line'))
    assert np.array_equal(acc.astype(np.float64), V.ref) and set(np.unique(acc)) == {0.0, 5.0}


def test_view_weights_one_key_contended_by_the_whole_wave(L):
    case = K.contended_case()
    _note('view_weight', G.check_view(sums_of(case), host(accumulate(L, case)), '(2, 2, 2), 200 samples'))


def test_view_weights_when_the_table_overflows(L):
    """512 distinct keys in one chunk, of which at least 47 find no slot in any insertion order (host test): the weights
    that take the fall-back must arrive like the others."""
    case = K.overflow_case()
    _note('view_weight', G.check_view(sums_of(case), host(accumulate(L, case)), 'overflow'))


def test_two_views_with_a_commit_in_between(L):
    a, b = K.view_case(256, 200), K.view_case(5, 65)
    n = int(np.prod(K.VIEW_DIMS))
    count = torch.zeros(n, device='cuda')
    acc = accumulate(L, a)
    Va, Vb = sums_of(a), sums_of(b)
    _note('view_weight', G.check_view(Va, host(acc), 'first view'))
    L.call('dvgo_view_count_commit', acc, count, n, L.stream_of(acc))
    assert int(torch.count_nonzero(acc)) == 0 and not bool(torch.any(torch.signbit(acc)))
    accumulate(L, b, acc)
    _note('view_weight', G.check_view(Vb, host(acc), 'second view, after the commit'))      # starts from exact zeros
    L.call('dvgo_view_count_commit', acc, count, n, L.stream_of(acc))
    G.check_counts([Va, Vb], host(count), 'two views')


@pytest.mark.parametrize('n_vox', [1, 256, 257])
def test_view_count_commit_is_exact(L, n_vox):
    one_up, one_dn = np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(1), np.float32(0))
    vals = np.array([37.5, 0.0, 1.0, one_up, one_dn, -0.0], np.float32)
    adds = np.array([1.0, 0.0, 0.0, 1.0, 0.0, 0.0], np.float32)
    idx = np.arange(n_vox) % 6
    acc, count0 = cu(vals[idx]), np.arange(n_vox, dtype=np.float32) % 3
    count = cu(count0)
    L.call('dvgo_view_count_commit', acc, count, n_vox, L.stream_of(acc))
    assert np.array_equal(host(count), count0 + adds[idx])
    got = host(acc)
    assert np.all(got == 0)
    guard = torch.full((n_vox + 2,), 2.0, device='cuda')                          # one past the end stays
    c2 = torch.zeros(n_vox + 1, device='cuda')
    L.call('dvgo_view_count_commit', guard, c2, n_vox, L.stream_of(acc))
    assert float(guard[n_vox]) == 2.0 and float(guard[n_vox + 1]) == 2.0 and float(c2[n_vox]) == 0.0 and bool(torch.all(c2[:n_vox] == 1))


def test_voxel_count_views_every_determined_voxel_is_exact():
    from directvoxgo_amd.dvgo import DirectVoxGO
    case = K.count_case()
    m = DirectVoxGO(K.COUNT_MIN, K.COUNT_MAX, num_voxels=K.COUNT_VOXELS, num_voxels_base=K.COUNT_VOXELS, alpha_init=1e-6).cuda()
    assert tuple(m.world_size.tolist()) == K.COUNT_DIMS and float(m.voxel_size) == case['voxel_size']
    ro, rd = cu(case['rays_o']), cu(case['rays_d'])
    cnt = m.voxel_count_views(rays_o_tr=ro, rays_d_tr=rd, imsz=[1] * K.COUNT_VIEWS, near=K.COUNT_NEAR, far=K.COUNT_FAR,
                              stepsize=K.COUNT_STEPSIZE, downrate=1)
    assert cnt.shape == m.density.shape
    views = []
    for v in range(K.COUNT_VIEWS):
        pos = G.view_positions(case['rays_o'][v], case['rays_d'][v], K.COUNT_MIN, K.COUNT_MAX, K.COUNT_NEAR, K.COUNT_FAR, case['step'],
                               case['n_samples'])
        views.append(G.view_sums(pos, K.COUNT_MIN, K.COUNT_MAX, K.COUNT_DIMS))
    G.check_counts(views, host(cnt), 'voxel_count_views')
    assert float(cnt.max()) == K.COUNT_VIEWS


# ------------------------------------------------------------------------------------------ segment sum
@pytest.mark.parametrize('C', [1, 3, 4])
def test_segment_sum(ops, L, C):
    case = K.segment_case(C)
    src, index, out0 = case['src'], case['index'], case['out0']
    S = G.segment_sums(src, index, out0)
    sq = (lambda a: a[:, 0]) if C == 1 else (lambda a: a)
    s, i, o = cu(sq(src)), cu(index), cu(sq(out0))
    got = ops.segment_coo(src=s, index=i, out=o, reduce='sum')
    assert same_bits(host(o), sq(out0))                                  # the op returns a new tensor, `out` is read only
    _note('segment_sum', G.check_segment(S, host(got), out0, 'segment_coo'))
    res = cu(out0)
    L.call('dvgo_segment_sum', cu(src), i, src.shape[0], C, out0.shape[0], res, L.stream_of(res))
    _note('segment_sum', G.check_segment(S, host(res), out0, 'dvgo_segment_sum'))
