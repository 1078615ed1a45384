"""CPU: directvoxgo_amd/pose.py (pure torch) and the host side of dvgo_grid_sample_bwd_xyz.

  se3_exp                against torch.linalg.matrix_exp of the 4x4 twist in float64, at |omega| in {0, 1e-6, 1e-4, 1, pi - 1e-3};
                         gradcheck at 0 and at a generic point
  CameraRefiner.rays     equal to render.get_rays at delta = 0 for the eight inverse_y / flip_x / flip_y combinations; its
                         Jacobian w.r.t. delta against float64 autograd of a direct restatement
  refine_poses           raises NotImplementedError for the four model kinds it does not differentiate
  the ABI                the header declares the entry, _lib types it, and its validation answers before any launch
"""
import ctypes
import itertools
import math
import os

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _twist(xi):
    """[n,6] -> the 4x4 twist matrices [n,4,4]"""
    n = xi.shape[0]
    T = torch.zeros(n, 4, 4, dtype=xi.dtype)
    w, v = xi[:, :3], xi[:, 3:]
    T[:, 0, 1], T[:, 0, 2], T[:, 1, 0], T[:, 1, 2], T[:, 2, 0], T[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    T[:, :3, 3] = v
    return T


@pytest.mark.parametrize('theta', [0.0, 1e-6, 1e-4, 0.99e-4, 1.0, math.pi - 1e-3])
def test_se3_exp_equals_the_matrix_exponential(theta):
    from directvoxgo_amd.pose import se3_exp
    gen = torch.Generator().manual_seed(3)
    axis = torch.randn(5, 3, generator=gen, dtype=torch.float64)
    axis = axis / axis.norm(dim=-1, keepdim=True)
    xi = torch.cat([axis * theta, torch.randn(5, 3, generator=gen, dtype=torch.float64)], -1)
    got = se3_exp(xi)
    want = torch.linalg.matrix_exp(_twist(xi))[:, :3, :]
    assert got.shape == (5, 3, 4) and got.dtype == torch.float64
    assert torch.allclose(got, want, rtol=0, atol=1e-13), float((got - want).abs().max())
    R = got[:, :, :3]
    assert torch.allclose(R @ R.transpose(1, 2), torch.eye(3, dtype=torch.float64).expand(5, 3, 3), atol=1e-13)


def test_se3_exp_gradient_at_zero_and_at_a_generic_point():
    from directvoxgo_amd.pose import se3_exp
    zero = torch.zeros(2, 6, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(se3_exp, (zero,), eps=1e-6, atol=1e-7)
    # first order at 0: d R / d omega = hat(e_k), d t / d v = I
    J = torch.autograd.functional.jacobian(se3_exp, torch.zeros(1, 6, dtype=torch.float64))[0, :, :, 0, :]     # [3,4,6]
    assert torch.isfinite(J).all()
    assert torch.equal(J[:, 3, 3:], torch.eye(3, dtype=torch.float64))
    assert J[2, 1, 0] == 1 and J[1, 2, 0] == -1 and J[0, 2, 1] == 1 and J[1, 0, 2] == 1
    gen = torch.Generator().manual_seed(4)
    x = (torch.randn(3, 6, generator=gen, dtype=torch.float64) * 0.7).requires_grad_()
    assert torch.autograd.gradcheck(se3_exp, (x,), eps=1e-6, atol=1e-7)
    f32 = se3_exp(torch.zeros(1, 6, requires_grad=True))
    f32.sum().backward()                                   # (float32 at 0: finite, too)
    assert f32.dtype == torch.float32


@pytest.mark.parametrize('theta', [1e-4, 1e-3, 1e-2, 0.1])
def test_se3_exp_float32_gradient_holds_between_the_series_and_the_closed_forms(theta):
    """`delta` is a float32 parameter that starts at 0 and passes through 1e-4 .. 1e-2 while it is refined.  The Jacobian's
    entries are at most about 1 + |v|; a float32 evaluation of a few dozen well-conditioned operations is allowed 64 u of
    that (u = 2^-24).  (theta - sin theta) / theta^3 in its closed form misses it by orders of magnitude here.)"""
    from directvoxgo_amd.pose import se3_exp
    gen = torch.Generator().manual_seed(6)
    axis = torch.randn(4, 3, generator=gen, dtype=torch.float64)
    axis = axis / axis.norm(dim=-1, keepdim=True)
    xi32 = torch.cat([axis * theta, torch.randn(4, 3, generator=gen, dtype=torch.float64)], -1).float()
    J32 = torch.autograd.functional.jacobian(se3_exp, xi32)
    J64 = torch.autograd.functional.jacobian(se3_exp, xi32.double())
    assert J32.dtype == torch.float32 and torch.isfinite(J32).all()
    scale = 1 + float(xi32[:, 3:].abs().max())
    assert float((J32.double() - J64).abs().max()) <= 64 * 2.0 ** -24 * scale
    assert float((se3_exp(xi32).double() - se3_exp(xi32.double())).abs().max()) <= 16 * 2.0 ** -24 * scale


H, W = 5, 7
K = np.array([[6.5, 0, 3.1], [0, 6.1, 2.2], [0, 0, 1]], np.float32)         # cx, cy off-centre


def _poses(n, seed=0):
    from directvoxgo_amd.scenes import pose_spherical
    gen = torch.Generator().manual_seed(seed)
    return torch.stack([pose_spherical(float(torch.rand(1, generator=gen)) * 360 - 180, -30.0 - 10 * v, 4.0 + 0.1 * v)[:3, :4]
                        for v in range(n)])


@pytest.mark.parametrize('inverse_y,flip_x,flip_y', list(itertools.product([False, True], repeat=3)))
def test_rays_equal_get_rays_at_zero_delta(inverse_y, flip_x, flip_y):
    from directvoxgo_amd.pose import CameraRefiner
    from directvoxgo_amd.render import get_rays
    poses = _poses(3)
    ref = CameraRefiner(poses, [[H, W]] * 3, [K] * 3, inverse_y=inverse_y, flip_x=flip_x, flip_y=flip_y)
    assert [tuple(p.shape) for p in ref.parameters()] == [(3, 6)] and float(ref.delta.detach().abs().sum()) == 0
    assert torch.equal(ref.poses(), poses)
    gen = torch.Generator().manual_seed(1)
    view = torch.randint(3, (40,), generator=gen)
    pi, pj = torch.randint(W, (40,), generator=gen), torch.randint(H, (40,), generator=gen)
    o, d, vd = ref.rays(view, pi, pj)
    assert not vd.requires_grad and o.requires_grad and d.requires_grad
    for v in range(3):
        ro, rd = get_rays(H, W, K, poses[v], inverse_y=inverse_y, flip_x=flip_x, flip_y=flip_y, mode='center')
        sel = view == v
        assert torch.equal(o[sel], ro[pj[sel], pi[sel]]) and torch.equal(d[sel], rd[pj[sel], pi[sel]])
        assert torch.equal(vd[sel], (rd / rd.norm(dim=-1, keepdim=True))[pj[sel], pi[sel]])
    with pytest.raises(NotImplementedError, match='NDC'):
        ref.rays(view, pi, pj, ndc=True)


def test_rays_jacobian_matches_a_direct_restatement():
    """float64 autograd of R' = expm(hat(omega)) R, t' = expm(twist) applied to t, rays = R' dirs, written without pose.py"""
    from directvoxgo_amd.pose import CameraRefiner
    poses = _poses(2, seed=5).double()
    ref = CameraRefiner(poses, [[H, W]] * 2, [K] * 2).double()
    gen = torch.Generator().manual_seed(2)
    delta = torch.randn(2, 6, generator=gen, dtype=torch.float64) * 0.05
    view = torch.tensor([0, 1, 1, 0])
    pi, pj = torch.tensor([0, 6, 3, 2]), torch.tensor([4, 0, 2, 1])

    def mine(dl):
        ref.delta.data = dl.detach().clone()
        return torch.autograd.functional.jacobian(lambda x: _with_delta(ref, x, view, pi, pj), dl)

    def direct(dl):
        T = torch.linalg.matrix_exp(_twist(dl))                              # [2,4,4]
        c2w = torch.cat([poses, torch.tensor([[[0, 0, 0, 1.0]]], dtype=torch.float64).expand(2, 1, 4)], 1)
        P = (T @ c2w)[view]
        dirs = torch.stack([(pi.double() + 0.5 - float(K[0, 2])) / float(K[0, 0]), -(pj.double() + 0.5 - float(K[1, 2])) / float(K[1, 1]),
                            -torch.ones(4, dtype=torch.float64)], -1)
        return torch.cat([P[:, :3, 3], (P[:, :3, :3] @ dirs.unsqueeze(-1)).squeeze(-1)], -1)

    J0, J1 = mine(delta), torch.autograd.functional.jacobian(direct, delta)
    assert J0.shape == J1.shape == (4, 6, 2, 6)
    assert torch.allclose(J0, J1, rtol=0, atol=1e-12), float((J0 - J1).abs().max())
    assert torch.allclose(_with_delta(ref, delta, view, pi, pj), direct(delta), rtol=0, atol=1e-13)


def _with_delta(ref, x, view, pi, pj):
    saved = ref.delta
    try:
        del ref.delta
        ref.delta = x                       # a plain tensor in the parameter's place: rays() is a function of it
        o, d, _ = ref.rays(view, pi, pj)
    finally:
        del ref.delta
        ref.delta = saved
    return torch.cat([o, d], -1)


def _unsupported():
    from directvoxgo_amd.dcvgo import DirectContractedVoxGO
    from directvoxgo_amd.dmpigo import DirectMPIGO
    from directvoxgo_amd.dvgo import DirectVoxGO
    from directvoxgo_amd.triplane import TriPlaneVoxGO
    kw = dict(num_voxels=8 ** 3, num_voxels_base=8 ** 3, alpha_init=1e-2)
    return {
        'DirectMPIGO': lambda: DirectMPIGO([-1, -1, 0], [1, 1, 1], num_voxels=8 ** 3, mpi_depth=8),
        'DirectContractedVoxGO': lambda: DirectContractedVoxGO([-1, -1, -1], [1, 1, 1], **kw),
        'TriPlaneVoxGO': lambda: TriPlaneVoxGO([-1, -1, -1], [1, 1, 1], **kw),
        'posbase_pe': lambda: DirectVoxGO([-1, -1, -1], [1, 1, 1], rgbnet_dim=12, posbase_pe=5, **kw),
    }


@pytest.mark.parametrize('kind', ['DirectMPIGO', 'DirectContractedVoxGO', 'TriPlaneVoxGO', 'posbase_pe'])
def test_refine_poses_names_the_model_it_cannot_differentiate(kind):
    from directvoxgo_amd.pose import CameraRefiner, refine_poses
    from directvoxgo_amd.train import FINE_TRAIN
    model = _unsupported()[kind]()
    ref = CameraRefiner(_poses(1), [[H, W]], [K])
    with pytest.raises(NotImplementedError, match=kind):
        refine_poses(model, ref, torch.zeros(1, H, W, 3), FINE_TRAIN, dict(near=0.1, far=1.0, stepsize=0.5, bg=1), 1, 8, 1e-3)


def test_header_declares_the_entry_and_lib_types_it():
    from directvoxgo_amd import _lib, build
    assert 'grid_sample_xyz.hip' in build.SOURCES
    build.build(verbose=False)
    with open(_lib.HEADER_PATH) as f:
        decl = _lib.declarations(f.read())
    restype, argtypes = decl['dvgo_grid_sample_bwd_xyz']
    P, i, q = _lib._Pointer, ctypes.c_int, ctypes.c_int64
    assert restype is ctypes.c_int and argtypes == [P, i, i, i, i, q, q, q, q, P, P, P, P, q, P, P]
    fn = _lib.lib().dvgo_grid_sample_bwd_xyz
    assert fn.argtypes == argtypes and _lib.ABI_VERSION == _lib.lib().dvgo_abi_version() >= 9


def test_validation_answers_before_any_launch():
    """-1 for a negative count or null pointers, 0 for an empty input, -2 past the 32-bit launch range: none of them
    touches the device, which is what makes the calls safe on a host without a GPU."""
    from directvoxgo_amd import _lib
    fn = _lib.lib().dvgo_grid_sample_bwd_xyz
    null, one = None, ctypes.c_void_p(16)          # any non-null value: rejected on size before it could be dereferenced
    geom = (1, 3, 4, 5, 60, 20, 5, 1)
    assert fn(null, *geom, null, null, null, null, -1, null, null) == -1
    assert fn(one, *geom, one, one, one, one, -1, one, null) == -1
    assert fn(null, *geom, null, null, null, null, 0, null, null) == 0
    assert fn(null, *geom, null, null, null, null, 8, null, null) == -1
    assert fn(one, *geom, one, one, one, one, 8, null, null) == -1                         # each pointer is looked at
    assert fn(one, 1, 0, 4, 5, 60, 20, 5, 1, one, one, one, one, 8, one, null) == -1       # an axis < 1
    assert fn(one, *geom, one, one, one, one, 1 << 31, one, null) == -2
    assert fn(one, 12, 3, 4, 5, 1, 240, 60, 12, one, one, one, one, 1 << 28, one, null) == -2   # M * C
    with pytest.raises(RuntimeError, match='invalid argument'):
        _lib.call('dvgo_grid_sample_bwd_xyz', None, *geom, None, None, None, None, -1, None, None)
