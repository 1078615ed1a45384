"""CPU: tests/raygrad_oracle.py held to its own references.

  * its formula, fed float64 cells and weights, equals float64 torch autograd of F.grid_sample (align_corners=True, zero
    padding, the reference's flipped ind_norm) at points whose float32 and float64 cells agree, points outside the box
    included;
  * on a lattice plane it gives the upper cell's derivative;
  * it catches a dropped corner, a flipped sign on one axis and a missing scale planted into a correct float32 evaluation;
  * the unplanted float32 evaluation, in the kernel's stated order, stays inside the bound on every record.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import raygrad_oracle as R


def torch_grad(grid, gout, xyz, mn, mx):
    """float64 torch autograd: d sum(gout * grid_sample(grid, xyz)) / d xyz -> [M,3]"""
    g = torch.from_numpy(np.asarray(grid, np.float64))[None]
    x = torch.from_numpy(np.asarray(xyz, np.float64)).requires_grad_()
    mn, mx = torch.from_numpy(np.asarray(mn, np.float64)), torch.from_numpy(np.asarray(mx, np.float64))
    ind = ((x - mn) / (mx - mn)).flip(-1) * 2 - 1
    out = F.grid_sample(g, ind.reshape(1, 1, 1, -1, 3), mode='bilinear', align_corners=True)
    out = out.reshape(g.shape[1], -1).T
    (gx,) = torch.autograd.grad(out, x, torch.from_numpy(np.asarray(gout, np.float64)))
    return gx.numpy()


def _agreeing(xyz, dims):
    """rows whose float32 and float64 cells agree (the float32 position is the input of both)"""
    a, b = R.inputs32(xyz, R.MN, R.MX, dims), R.inputs64(xyz.astype(np.float64), R.MN, R.MX, dims)
    return np.all(a.ijk0 == b.ijk0, -1)


@pytest.mark.parametrize('C,layout,dims,offset', R.GRIDS)
def test_formula_equals_torch_autograd_in_float64(C, layout, dims, offset):
    xyz = R.points(dims, 4000, seed=11)
    keep = _agreeing(xyz, dims)
    assert keep.sum() > 3000
    xyz = xyz[keep]
    I = R.inputs64(xyz.astype(np.float64), R.MN, R.MX, dims)
    outside = ~np.all(I.inb, -1)
    assert outside.sum() > 500 and (~np.any(I.inb, -1)).sum() > 100          # padded corners and fully outside points
    grid, gout = R.grid_values(C, dims, 3), R.grad_values(xyz.shape[0], C, 4)
    S = R.sums(grid, gout, I, R.scale(R.MN, R.MX, dims))
    want = torch_grad(grid, gout, xyz, R.MN, R.MX)
    assert np.all(np.abs(S.ref - want) <= 1e-13 * (S.mag + 1.0)), float(np.abs(S.ref - want).max())
    assert np.all(want[S.mag == 0] == 0)


def test_lattice_plane_takes_the_upper_cell():
    dims = (5, 4, 3)
    mn, mx = np.zeros(3, np.float32), np.array([4, 3, 2], np.float32)        # world == grid index, exactly
    h = np.array([0.0, 1.0, 4.0, 9.0, 16.0])
    grid = np.broadcast_to(h[None, :, None, None], (1, *dims)).astype(np.float32).copy()
    xyz = np.array([[k, 1.25, 0.5] for k in range(5)], np.float32)           # on the planes x = 0 .. 4
    for I in (R.inputs32(xyz, mn, mx, dims), R.inputs64(xyz, mn, mx, dims)):
        assert np.array_equal(I.ijk0[:, 0], np.arange(5))
        S = R.sums(grid, np.ones((5, 1), np.float32), I, R.scale(mn, mx, dims))
        # the upper cell's slope h[k + 1] - h[k]; at the last node the upper cell is outside (zero padding): 0 - h[4]
        assert np.allclose(S.ref[:, 0], [1, 3, 5, 7, -16], atol=1e-12)
        assert np.allclose(S.ref[:, 1:], 0, atol=1e-12)
    assert np.allclose(torch_grad(grid, np.ones((5, 1)), xyz, mn, mx)[:, 0], [1, 3, 5, 7, -16], atol=1e-12)


@pytest.fixture(scope='module', params=R.GRIDS[:5], ids=lambda g: f'C{g[0]}-{g[1]}-{g[2]}-{g[3]}')
def case(request):
    C, _, dims, _ = request.param
    xyz = R.points(dims, 257, seed=5)
    I = R.inputs32(xyz, R.MN, R.MX, dims)
    grid, gout = R.grid_values(C, dims, 6), R.grad_values(257, C, 7)
    return dims, I, grid, gout, R.sums(grid, gout, I, R.scale(R.MN, R.MX, dims))


def test_float32_evaluation_in_the_stated_order_is_inside_the_bound(case):
    dims, I, grid, gout, S = case
    r = R.check(S, R.evaluate32(grid, gout, I, R.MN, R.MX, dims))
    assert 0 < r <= 1


def test_unit_axis_and_padded_points_are_exact_zeros():
    C, _, dims, _ = R.GRIDS[5]
    xyz = R.points(dims, 257, seed=5)
    I = R.inputs32(xyz, R.MN, R.MX, dims)
    grid, gout = R.grid_values(C, dims, 6), R.grad_values(257, C, 7)
    S = R.sums(grid, gout, I, R.scale(R.MN, R.MX, dims))
    assert np.all(S.mag[:, 0] == 0) and np.any(S.mag[:, 1] > 0)
    got = R.evaluate32(grid, gout, I, R.MN, R.MX, dims)
    R.check(S, got)
    got[3, 0] = 1e-30
    with pytest.raises(AssertionError, match='nothing contributes'):
        R.check(S, got)


@pytest.mark.parametrize('mutation', [dict(drop_corner=0), dict(drop_corner=5), dict(flip_axis=0), dict(flip_axis=1),
                                      dict(flip_axis=2), dict(no_scale=True)], ids=str)
def test_oracle_catches_planted_mistakes(case, mutation):
    dims, I, grid, gout, S = case
    with pytest.raises(AssertionError, match='outside gamma'):
        R.check(S, R.evaluate32(grid, gout, I, R.MN, R.MX, dims, **mutation))


def test_unwritten_rows_are_reported(case):
    dims, I, grid, gout, S = case
    got = R.evaluate32(grid, gout, I, R.MN, R.MX, dims)
    got[100] = np.nan
    with pytest.raises(AssertionError, match='non-finite'):
        R.check(S, got)
