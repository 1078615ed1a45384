"""CPU: the plane regulariser's oracle (tests/plane_tv_oracle.py), float32 form against float64 form on the GPU test's
inputs; the C entry's answers before any launch; and the host side of the model method and of TrainStep's config keys.

Error bound of the float32 form against the float64 form, U = 2^-24, A = |g0| + sum |w * clamp| + |wl1|:
    |reg32 - reg64| <= 8 U A      on every element.
Derivation: at most 5 terms, each carrying one subtraction rounding and one product rounding (the L1 term: one product
rounding only), and clamp1 never enlarges an error: at most 2 U times the term's magnitude each, 2 U A in all.  Then at
most 6 additions (g + term five times, the first of them onto an exact 0, and g0 + g), each rounding a partial sum that
is no larger than A: at most 5 U A.  Together 7 U A, rounded up to 8 U A for the second-order terms.  No element is
excluded.
"""
import ctypes

import numpy as np
import pytest
import torch

import plane_tv_oracle as PO


def _check(tensors, weights, dense):
    worst = 0.0
    for (p, g), (wh, ww, wl1) in zip(tensors, weights):
        got = PO.reg32(p, g, wh, ww, wl1, dense).astype(np.float64)
        ref, A = PO.reg64(p, g, wh, ww, wl1, dense)
        err, bound = np.abs(got - ref), 8 * PO.U * A
        assert (err <= bound).all(), float((err - bound).max())
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    return worst


@pytest.mark.parametrize('l1', [False, True])
@pytest.mark.parametrize('dense', [True, False])
@pytest.mark.parametrize('R', [1, 3, 16])
def test_float32_form_within_8UA_of_the_float64_form(R, dense, l1):
    worst = _check(PO.six(R, 100 + R), PO.weights_of(6, l1), dense)
    print(f'R={R} dense={dense} l1={l1}: worst err / bound {worst:.3f}')
    assert worst > 0                                                   # (the two forms are not the same computation)


@pytest.mark.parametrize('dense', [True, False])
def test_float32_form_within_8UA_on_the_larger_case(dense):
    print('worst err / bound', _check(PO.big(7), PO.weights_of(3, True), dense))


def test_inputs_cover_the_edge_cases():
    """The clamp is active on part of the differences and idle on part; equal neighbours, exact zeros of both signs in the
    parameters; about half of the gradients zero, some of them -0.0; sparse mode keeps those bits, dense mode moves them."""
    for R in (3, 16):
        for (p, g), (wh, ww, wl1) in zip(PO.six(R, 100 + R), PO.weights_of(6, True)):
            for d in ([np.abs(p[:, 1:] - p[:, :-1])] if p.shape[1] > 1 else []) + ([np.abs(p[:, :, 1:] - p[:, :, :-1])] if p.shape[2] > 1 else []):
                assert (d > 1).any() and (d < 1).any() and (d == 0).any()
            zero = g == 0
            if p.size < 32:                                                   # (the line of one node: R values in all)
                continue
            assert (p == 0).any()
            assert 0.3 < zero.mean() < 0.7 and (np.signbit(g) & zero).any() and (~np.signbit(g) & zero).any()
            sparse, dense = PO.reg32(p, g, wh, ww, wl1, False), PO.reg32(p, g, wh, ww, wl1, True)
            assert np.array_equal(sparse[zero].view(np.uint32), g[zero].view(np.uint32))
            assert np.array_equal(sparse[~zero], dense[~zero]) and (dense[zero] != 0).any()
    p, g = PO.six(16, 116)[0]
    assert (p.reshape(-1).view(np.uint32) == 0x80000000).any()                # a -0.0 parameter: sgn gives 0
    # a line of one node has no neighbour: only L1 moves it
    p, g = np.float32([[[2.0]]]), np.float32([[[0.5]]])
    assert PO.reg32(p, g, 0.7, 0.7, 0.0, True)[0, 0, 0] == np.float32(0.5)
    assert PO.reg32(p, g, 0.7, 0.7, 0.25, True)[0, 0, 0] == np.float32(0.75)


def test_oracle_is_the_gradient_of_the_clamped_tv_where_the_clamp_is_idle():
    """With every |difference| < 1 and wl1 = 0 the stencil is the gradient of w * sum of squared neighbour differences
    (each pair counted once): a float64 autograd restatement, rtol 1e-12."""
    rng = np.random.default_rng(3)
    p = (0.2 * rng.standard_normal((4, 6, 5))).astype(np.float32)
    g0 = rng.standard_normal(p.shape).astype(np.float32)
    wh, ww = 0.4, 0.9
    t = torch.from_numpy(p).double().requires_grad_()
    loss = float(np.float32(ww)) * (t[:, :, 1:] - t[:, :, :-1]).pow(2).sum() + float(np.float32(wh)) * (t[:, 1:] - t[:, :-1]).pow(2).sum()
    loss.backward()
    ref, _ = PO.reg64(p, g0, wh, ww, 0.0, True)
    np.testing.assert_allclose(ref - g0.astype(np.float64), 0.5 * t.grad.numpy(), rtol=1e-12, atol=1e-15)


# ---------------------------------------------------------------------------------------------- build, typing, validation
@pytest.fixture(scope='module')
def lib():
    from directvoxgo_amd import _lib, build
    assert 'plane_tv.hip' in build.SOURCES
    build.build(verbose=False)
    return _lib.lib()


def test_typing(lib):
    from directvoxgo_amd import _lib
    with open(_lib.HEADER_PATH) as f:
        decl = _lib.declarations(f.read())
    P, i = _lib._Pointer, ctypes.c_int
    assert decl['dvgo_plane_reg_add_grad'] == (ctypes.c_int, [P, P, P, P, P, i, i, P])
    assert lib.dvgo_plane_reg_add_grad.argtypes == decl['dvgo_plane_reg_add_grad'][1]
    assert _lib.ABI_VERSION == lib.dvgo_abi_version() == 11


def _call(lib, n, sizes=None, null_param=None, null_grad=None, tables=True, dense=1):
    m = max(n, 1)
    one = 16          # any non-null value: rejected before it could be dereferenced, or never reached
    sizes = sizes or [(4, 5, 6)] * m
    vp = lambda skip: (ctypes.c_void_p * m)(*[None if k == skip else one for k in range(m)])       # noqa: E731
    sz = (ctypes.c_int64 * (3 * m))(*[v for s in sizes for v in s])
    st = (ctypes.c_int64 * (3 * m))(*[v for (C, H, W) in sizes for v in (1, W * C, C)])
    wt = (ctypes.c_float * (3 * m))(*([0.5] * (3 * m)))
    if not tables:
        return lib.dvgo_plane_reg_add_grad(None, None, None, None, None, n, dense, None)
    return lib.dvgo_plane_reg_add_grad(vp(null_param), vp(null_grad), sz, st, wt, n, dense, None)


def test_entry_point_validates_before_any_launch(lib):
    assert _call(lib, -1) == -1 and _call(lib, 9) == -1
    assert _call(lib, 0) == 0 and _call(lib, 0, tables=False) == 0                  # nothing to do: no table is looked at
    assert _call(lib, 3, tables=False) == -1                                        # a null table
    for which in range(5):                                                          # ... each of the five
        args = [(ctypes.c_void_p * 1)(16), (ctypes.c_void_p * 1)(16), (ctypes.c_int64 * 3)(2, 3, 4), (ctypes.c_int64 * 3)(1, 8, 2),
                (ctypes.c_float * 3)(0.5, 0.5, 0.0)]
        args[which] = None
        assert lib.dvgo_plane_reg_add_grad(*args, 1, 1, None) == -1, which
    for bad in ((0, 5, 6), (4, 0, 6), (4, 5, 0), (4, -5, 6)):                       # a size below 1
        assert _call(lib, 2, sizes=[(4, 5, 6), bad]) == -1, bad
    assert _call(lib, 8, null_param=7) == -1 and _call(lib, 8, null_grad=0) == -1   # a null tensor pointer
    assert _call(lib, 1, null_param=0, dense=0) == -1
    # index types: a tensor of 2^31 elements, and 2^31 rows in all (8 channels-last tensors of 2^28 rows each)
    assert _call(lib, 1, sizes=[(1 << 11, 1 << 10, 1 << 10)]) == -2
    assert _call(lib, 8, sizes=[(1, 1 << 28, 2)] * 8) == -2
    assert _call(lib, 2, sizes=[(1 << 11, 1 << 10, 1 << 10), (4, 0, 6)]) == -1      # an invalid argument outranks a size
    from directvoxgo_amd import _lib
    with pytest.raises(RuntimeError, match='invalid argument'):               # the typed call turns the code into an error
        _lib.call('dvgo_plane_reg_add_grad', None, None, None, None, None, 2, 1, None)


def test_op_rejects_cpu_tensors_and_mismatched_arguments():
    from directvoxgo_amd.ops import plane_reg_add_grad
    p = torch.zeros(1, 4, 5, 6)
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        plane_reg_add_grad([p], [torch.zeros_like(p)], [(0.1, 0.1, 0.0)], True)
    with pytest.raises(ValueError, match='1 params, 2 grads'):
        plane_reg_add_grad([p], [p, p], [(0.1, 0.1, 0.0)], True)
    plane_reg_add_grad([], [], [], True)                                            # an empty list is a no-op


# ---------------------------------------------------------------------------------------------- models and TrainStep, host side
BASE = dict(num_voxels=10 * 12 * 14, num_voxels_base=16 ** 3, alpha_init=1e-2, fast_color_thres=1e-4)
BOX = ([-1.0, -1.2, -1.4], [1.0, 1.2, 1.4])
RK = dict(near=0.5, far=6.0, bg=1, stepsize=0.5)


def test_model_method_refuses_line_weights_on_the_base_class():
    from directvoxgo_amd.triplane import TriPlaneVoxGO
    m = TriPlaneVoxGO(*BOX, **BASE)
    with pytest.raises(ValueError, match='no lines'):
        m.plane_regularizers_add_grad(True, weight_tv_planes=1.0, weight_tv_lines=1e-3)
    with pytest.raises(ValueError, match='no lines'):
        m.plane_regularizers_add_grad(False, weight_l1_lines=1e-3)
    m.plane_regularizers_add_grad(True)                                 # all weights zero: nothing to do, no device needed
    m.plane_regularizers_add_grad(False, weight_tv_planes=1.0)          # sparse, no .grad anywhere: every tensor is skipped
    assert all(p.grad is None for p in m.planes.values())
    with pytest.raises(NotImplementedError, match='k0'):                # (unchanged)
        m.k0_total_variation_add_grad(1.0, True)


def test_model_weights_follow_the_stated_normalisation():
    from directvoxgo_amd.vm import VMTriPlaneVoxGO
    m = VMTriPlaneVoxGO(*BOX, n_comp=4, **BASE)
    items = m._plane_reg_items(2.0, 3.0, 0.5)
    assert [id(p) for p, _ in items] == [id(m.planes[k]) for k in PO.KEYS] + [id(m.lines[k]) for k in PO.KEYS]
    for k, (p, (wh, ww, wl1)) in zip(PO.KEYS, items[:3]):
        H, W = p.shape[2:]
        assert wh == ww == 2.0 * max(H, W) / 128 / 4 and wl1 == 0
    for k, (ln, (wh, ww, wl1)) in zip(PO.KEYS, items[3:]):
        assert wh == 3.0 * ln.shape[2] / 128 / 2 and ww == 0 and wl1 == 0.5           # L1 is not scaled by resolution
    assert len(m._plane_reg_items(2.0, 0.0, 0.0)) == 3 and m._plane_reg_items(0.0, 0.0, 0.0) == []
    assert len(m._plane_reg_items(0.0, 0.0, 0.5)) == 3


def test_train_step_refuses_the_keys_on_models_that_cannot_honour_them():
    from directvoxgo_amd.dvgo import DirectVoxGO
    from directvoxgo_amd.train import FINE_TRAIN, TrainStep
    from directvoxgo_amd.triplane import TRI_FINE_TRAIN, TriPlaneVoxGO
    from directvoxgo_amd.vm import VM_FINE_TRAIN, VMTriPlaneVoxGO
    dv = DirectVoxGO(*BOX, **BASE)
    with pytest.raises(ValueError, match='weight_tv_planes'):
        TrainStep(dv, dict(FINE_TRAIN, weight_tv_planes=1e-3), RK)
    tri = TriPlaneVoxGO(*BOX, **BASE)
    with pytest.raises(ValueError, match='no lines'):
        TrainStep(tri, dict(TRI_FINE_TRAIN, weight_tv_lines=1e-3), RK)
    with pytest.raises(ValueError, match='no lines'):
        TrainStep(tri, dict(TRI_FINE_TRAIN, weight_tv_planes=1e-3, weight_l1_lines=1e-3), RK)
    # configs without the keys construct as before, on every model, and plan no regulariser
    for model, cfg in ((dv, FINE_TRAIN), (tri, TRI_FINE_TRAIN), (VMTriPlaneVoxGO(*BOX, n_comp=4, **BASE), VM_FINE_TRAIN)):
        assert not any(k in cfg for k in ('weight_tv_planes', 'weight_tv_lines', 'weight_l1_lines'))
        step = TrainStep(model, dict(cfg), RK)
        assert not step.plane_reg_on and not step._tv_weighted()
        assert not step._plan(torch.zeros(4, 3), 1).tv
    # explicit zeros are the same as absent keys; the keys are legal where the model can honour them
    assert not TrainStep(dv, dict(FINE_TRAIN, weight_tv_planes=0.0, weight_tv_lines=0.0), RK).plane_reg_on
    assert TrainStep(tri, dict(TRI_FINE_TRAIN, weight_tv_planes=1e-3), RK).plane_reg_on


def test_plan_and_can_capture_count_the_new_keys():
    from directvoxgo_amd.train import TrainStep
    from directvoxgo_amd.vm import VM_FINE_TRAIN, VMTriPlaneVoxGO
    m = VMTriPlaneVoxGO(*BOX, n_comp=4, **BASE)
    cfg = dict(VM_FINE_TRAIN, tv_after=0, tv_before=3, tv_every=1, tv_dense_before=2, weight_l1_lines=1e-3)
    step = TrainStep(m, cfg, RK)
    rays = torch.zeros(4, 3)
    assert [step._plan(rays, s).tv for s in (0, 1, 2, 3, 4)] == [False, True, True, False, False]
    assert step._tv_weighted() and not step.can_capture()
    assert not TrainStep(m, dict(cfg, weight_l1_lines=0.0), RK)._plan(rays, 1).tv
    assert [TrainStep(m, dict(cfg, tv_every=2, tv_before=9), RK)._plan(rays, s).tv for s in (1, 2, 3, 4)] == [False, True, False, True]
