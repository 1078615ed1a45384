"""CPU: the vector-matrix samplers' position gradient (csrc/vm_xyz.hip) without a device.

  * tests/vm_raygrad_oracle.py's `ref` equals a central difference of a pure float64 forward (features and density) at cell
    interiors, inside the box and up to one cell outside it, and is exactly zero (`mag` too) further out and at a NaN;
  * the kernel's arithmetic restated in float32 numpy (interp_oracle.fma32) stays inside the bound the GPU test applies to the
    kernel, on every case of that test, and planted mistakes leave it: the bound holds for the reference alone;
  * at least half of the in-box outputs of those cases exceed 100 x their bound, so a kernel returning zeros cannot pass;
  * the boundary: the declarations parse, _lib types both entries, the library exports them, tp_check's staged order;
  * host logic: `raygrad` is no get_kwargs key and survives load_model, the default models' refusals name the class and
    carry the hint, refine_poses(fused=True) is a ValueError.
"""
import ctypes

import numpy as np
import pytest
import torch

import vm_raygrad_oracle as VR

f32 = np.float32


def _interior_points(shape, M, rng, lo=-0.08, hi=1.08):
    """Points at least 0.05 of a cell away from every lattice line of every plane and line of `shape`, between `lo` and
    `hi` box extents (0.08 of the box is less than one cell of every axis: the longest axis has 9 nodes)."""
    sizes, lens = VR.SHAPES[shape]
    counts = {a: set() for a in range(3)}
    for key in VR.KEYS:
        ah, aw = VR.TO.AXES[key]
        counts[ah].add(sizes[key][0]); counts[aw].add(sizes[key][1]); counts[VR.VO.LINE_AXIS[key]].add(lens[key])
    out = np.empty((M, 3))
    for a in range(3):
        col = np.empty(0)
        while col.size < M:
            u = rng.uniform(lo, hi, 4 * M)
            ok = np.ones(u.size, bool)
            for n in counts[a] - {1}:                      # (an axis of size 1 has no lattice line to stay away from)
                g = u * (n - 1)
                ok &= np.abs(g - np.round(g)) > 0.05
            col = np.concatenate([col, u[ok]])
        out[:, a] = col[:M]
    mn, mx = VR.MN.astype(np.float64), VR.MX.astype(np.float64)
    return (mn + out * (mx - mn)).astype(f32)


@pytest.mark.parametrize('shape', sorted(VR.SHAPES))
@pytest.mark.parametrize('density', [False, True])
def test_oracle_equals_a_central_difference_of_the_float64_forward(shape, density):
    rng = np.random.default_rng(11)
    R, M, h = 3, 300, 1e-6
    planes, lines = VR.tensors(shape, R, rng)
    xyz = _interior_points(shape, M, rng)
    gout = rng.standard_normal(M if density else (M, 3 * R)).astype(f32)
    S = VR.sums(planes, lines, gout, xyz, VR.MN, VR.MX)
    g64 = gout.astype(np.float64)
    outside = ~VR.in_box(xyz)
    assert outside.sum() > 20 and (S.mag[outside].max(1) > 0).all()          # less than one cell outside: not zero
    for a in range(3):
        d = np.zeros(3); d[a] = h
        x64 = xyz.astype(np.float64)
        diff = VR.forward64(planes, lines, x64 + d, VR.MN, VR.MX, density) - VR.forward64(planes, lines, x64 - d, VR.MN, VR.MX, density)
        fd = (diff * g64).sum(-1) / (2 * h) if not density else diff * g64 / (2 * h)
        # ref differs from the float64 derivative by the float32 rounding of the weights (2^-24 per weight, a few per
        # term) and the difference quotient by cancellation, 2^-53 / h = 1e-10 of the forward's magnitude
        err = np.abs(fd - S.ref[:, a])
        print(shape, density, a, 'worst', float((err / (1 + S.mag[:, a])).max()))
        assert (err <= 1e-5 * (1.0 + S.mag[:, a])).all(), a
    assert (S.mag >= np.abs(S.ref) - 1e-12).all()


def test_oracle_is_zero_beyond_one_cell_and_at_a_nan():
    rng = np.random.default_rng(12)
    planes, lines = VR.tensors('base', 4, rng)
    xyz = _interior_points('base', 60, rng, 0.1, 0.9)
    ext = (VR.MX - VR.MN)
    for m in range(48):
        a = m % 3
        xyz[m, a] = (VR.MX[a] + ext[a] * f32(0.6)) if m % 2 else (VR.MN[a] - ext[a] * f32(0.6))       # > one cell (<= 0.5 box)
    xyz[48, 2] = np.nan
    xyz[49] = np.nan
    for gout in (rng.standard_normal((60, 12)).astype(f32), rng.standard_normal(60).astype(f32)):
        S = VR.sums(planes, lines, gout, xyz, VR.MN, VR.MX)
        assert (S.mag[:50] == 0).all() and (S.ref[:50] == 0).all() and (S.mag[50:] > 0).all()
        got = VR.evaluate32(planes, lines, gout, xyz, VR.MN, VR.MX)
        assert (got[:50] == 0).all()
        VR.check(S, got)
    # an axis of size 1 has scale 0 on the plane (or line) it belongs to
    planes, lines = VR.tensors('N1', 4, rng)
    S = VR.sums(planes, lines, rng.standard_normal(60).astype(f32), xyz, VR.MN, VR.MX)
    assert S.mag[50:].min() > 0                                               # the other two planes still contribute


def _cases():
    """Every (shape, R, M) of the GPU test, with its inputs and both incoming gradients."""
    for shape in sorted(VR.SHAPES):
        for R in VR.RS:
            rng = np.random.default_rng(500 + R)
            planes, lines = VR.tensors(shape, R, rng)
            for M in VR.MS:
                xyz = VR.points(M, rng)
                yield shape, R, M, planes, lines, xyz, rng.standard_normal((M, 3 * R)).astype(f32), rng.standard_normal(M).astype(f32)


def test_float32_restatement_is_inside_the_bound_on_every_case_of_the_gpu_test():
    worst, share = 0.0, []
    for shape, R, M, planes, lines, xyz, g_feat, g_dens in _cases():
        g_dens[::7] = 0
        for gout in (g_feat, g_dens):
            S = VR.sums(planes, lines, gout, xyz, VR.MN, VR.MX)
            assert S.k() == R + 12
            worst = max(worst, VR.check(S, VR.evaluate32(planes, lines, gout, xyz, VR.MN, VR.MX), f'{shape} R={R} M={M}'))
            if M == 1000:
                inside = VR.in_box(xyz)
                if gout.ndim == 1:
                    inside &= gout != 0
                    assert (S.mag[gout == 0] == 0).all()
                big = np.abs(S.ref[inside]) > 100 * S.bound()[inside]
                # (an axis of size 1 contributes nothing on its plane or line; the other two still do)
                share.append(float(big.mean()))
                nan = np.isnan(xyz).any(1)
                assert nan.sum() == 2 and (S.mag[nan] == 0).all()
                with np.errstate(invalid='ignore'):
                    far = (np.abs((xyz - VR.MN) / (VR.MX - VR.MN) - 0.5) > 1.0).any(1)        # more than half a box outside:
                assert far.sum() >= 4                                                        # one cell of a 3-node axis
                if shape == 'base':                                                          # (an axis of size 1 is never left)
                    assert (S.mag[far] == 0).all()
    print('float32 restatement: worst err / bound', worst, '; least share of in-box outputs above 100 x bound', min(share))
    assert min(share) >= 0.5


def test_planted_mistakes_leave_the_bound():
    rng = np.random.default_rng(13)
    planes, lines = VR.tensors('base', 4, rng)
    xyz = VR.points(1000, rng)
    for gout in (rng.standard_normal((1000, 12)).astype(f32), rng.standard_normal(1000).astype(f32)):
        S = VR.sums(planes, lines, gout, xyz, VR.MN, VR.MX)
        VR.check(S, VR.evaluate32(planes, lines, gout, xyz, VR.MN, VR.MX))
        for planted in (dict(drop_corner=2), dict(flip='n'), dict(flip='hw'), dict(no_scale=True), dict(clamp=True)):
            with pytest.raises(AssertionError):
                VR.check(S, VR.evaluate32(planes, lines, gout, xyz, VR.MN, VR.MX, **planted))
        with pytest.raises(AssertionError, match='non-finite'):
            VR.check(S, np.full((1000, 3), np.nan, f32))
        with pytest.raises(AssertionError):
            VR.check(S, np.zeros((1000, 3), f32))


# ---------------------------------------------------------------------------------------------- boundary
ENTRIES = ('dvgo_vm_bwd_xyz', 'dvgo_vm_density_bwd_xyz')


@pytest.fixture(scope='module')
def lib():
    from directvoxgo_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def test_header_declares_both_entries_and_lib_types_them(lib):
    from directvoxgo_amd import _lib, build
    assert 'vm_xyz.hip' in build.SOURCES and 'vm.hip' in build.SOURCES and 'vm_density.hip' in build.SOURCES
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    decl = _lib.declarations(text)
    P, i, q = _lib._Pointer, ctypes.c_int, ctypes.c_int64
    sig = [P, i, i, q, q, q] * 3 + [P, i, q, q] * 3 + [i, P, P, P, P, q, P, P]
    for name in ENTRIES:
        assert decl[name] == (ctypes.c_int, sig), name
        assert getattr(lib, name).argtypes == sig and getattr(lib, name).restype is ctypes.c_int
        assert getattr(ctypes.CDLL(_lib.SO_PATH), name)                              # exported
    assert _lib.ABI_VERSION == lib.dvgo_abi_version() == 11                          # no bump
    assert 'the two dvgo_vm_*bwd_xyz entries were added' in text and 'Ah = fmaf(t, dh, Ah)' in text


KEYS = ('xy', 'yz', 'zx')
SIZES = ((6, 7), (3, 9), (8, 2))
POINTERS = KEYS + ('xy_line', 'yz_line', 'zx_line', 'xyz', 'mn', 'mx', 'gout', 'gxyz')
BIG = (1 << 31) // 12 + 1             # M * 3R >= 2^31 at R = 4


def _call(lib, name, M=8, R=4, sizes=SIZES, lines=(5, 1, 9), null=()):
    one = ctypes.c_void_p(16)         # any non-null value: rejected before it could be dereferenced, or never reached
    p = lambda k: None if k in null else one         # noqa: E731
    args = []
    for k, (H, W) in zip(KEYS, sizes):
        args += [p(k), H, W, 1, W * R, R]
    for k, N in zip(KEYS, lines):
        args += [p(k + '_line'), N, 1, R]
    return getattr(lib, name)(*args, R, p('gout'), p('xyz'), p('mn'), p('mx'), M, p('gxyz'), None)


@pytest.mark.parametrize('name', ENTRIES)
def test_entries_judge_their_arguments_in_tp_checks_order(lib, name):
    """tests/test_plane_entries_host.py's stages for dvgo_vm_fwd, with grad_out and grad_xyz among the pointers."""
    assert _call(lib, name, M=BIG) == -2                                             # the range alone
    assert _call(lib, name, M=BIG, sizes=((6, 7), (0, 9), (8, 2))) == -1             # shapes before the range
    assert _call(lib, name, M=BIG, lines=(0, 1, 9)) == -1 and _call(lib, name, M=0, lines=(5, 0, 9)) == -1
    assert _call(lib, name, M=-1) == -1 and _call(lib, name, R=-1) == -1
    for k in POINTERS:
        assert _call(lib, name, null=(k,)) == -1, k                                  # each pointer is looked at
        assert _call(lib, name, M=BIG, null=(k,)) == -1, k                           # NULL before the range
    assert _call(lib, name, M=BIG, R=0, null=POINTERS) == 0                          # nothing to do before NULL and the range
    assert _call(lib, name, M=0, null=POINTERS) == 0


def test_ops_reject_cpu_tensors_and_wrong_shapes():
    from directvoxgo_amd.ops import vm_bwd_xyz, vm_density, vm_density_bwd_xyz, vm_sample
    xyz, mn, mx = torch.zeros(7, 3, requires_grad=True), -torch.ones(3), torch.ones(3)
    planes = [torch.zeros(1, 4, 3, 5) for _ in range(3)]
    lines = [torch.zeros(1, 4, 6, 1) for _ in range(3)]
    for fn in (vm_sample, vm_density):
        with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
            fn(planes, lines, xyz, mn, mx, position_grad=True)
    for fn, g in ((vm_bwd_xyz, torch.zeros(7, 12)), (vm_density_bwd_xyz, torch.zeros(7))):
        with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
            fn(g, planes, lines, xyz.detach(), mn, mx)


# ---------------------------------------------------------------------------------------------- models and pose, host side
BASE = dict(num_voxels=10 * 12 * 14, num_voxels_base=16 ** 3, alpha_init=1e-2, fast_color_thres=1e-4)
BOX = ([-1.0, -1.2, -1.4], [1.0, 1.2, 1.4])
SMALL = dict(n_comp=4, rgbnet_dim=6, rgbnet_width=64)
RK = dict(near=0.1, far=1.0, stepsize=0.5, bg=1)


def _classes():
    from directvoxgo_amd.tensorf import TensoRFVoxGO
    from directvoxgo_amd.vm import VMTriPlaneVoxGO
    return VMTriPlaneVoxGO, TensoRFVoxGO


def _model(cls, **kw):
    extra = dict(density_n_comp=4) if cls.__name__ == 'TensoRFVoxGO' else {}
    return cls(*BOX, **{**BASE, **SMALL, **extra, **kw})


@pytest.mark.parametrize('which', [0, 1])
def test_raygrad_is_a_plain_attribute_and_survives_load_model(which, tmp_path):
    from directvoxgo_amd.checkpoint import load_model, save_checkpoint
    cls = _classes()[which]
    assert _model(cls).raygrad is False and _model(cls, raygrad=True).raygrad is True and _model(cls, raygrad=1).raygrad is True
    m = _model(cls, raygrad=True)
    kw = m.get_kwargs()
    assert 'raygrad' not in kw and set(kw) == set(_model(cls).get_kwargs()) and not any('raygrad' in k for k in m.state_dict())
    path = str(tmp_path / 'm.tar')
    save_checkpoint(path, m, None, 3)
    assert load_model(cls, path).raygrad is False
    m2 = load_model(cls, path, raygrad=True)
    assert m2.raygrad is True and set(m2.state_dict()) == set(m.state_dict()) and torch.equal(m2.planes['xy'], m.planes['xy'])


@pytest.mark.parametrize('which', [0, 1])
def test_refine_poses_accepts_only_the_model_with_raygrad(which):
    from directvoxgo_amd.pose import CameraRefiner, _supported, refine_poses
    from directvoxgo_amd.tensorf import TENSORF_FINE_TRAIN
    cls = _classes()[which]
    name = cls.__name__
    H = W = 4
    K = np.array([[4.0, 0, 2], [0, 4.0, 2], [0, 0, 1]], np.float32)
    ref = CameraRefiner(np.eye(4, dtype=np.float32)[None, :3], [[H, W]], [K])
    args = (ref, torch.zeros(1, H, W, 3), TENSORF_FINE_TRAIN, RK, 1, 8, 1e-3)
    assert not _supported(_model(cls)) and not _supported(_model(cls, fused=False))
    assert _supported(_model(cls, raygrad=True)) and _supported(_model(cls, raygrad=True, fused=False))
    with pytest.raises(NotImplementedError, match=f'refine_poses: {name} is not supported.*construct it with raygrad=True'):
        refine_poses(_model(cls), *args)
    for m in (_model(cls, raygrad=True), _model(cls, raygrad=True, fused=False)):      # before fused_raygrad is touched
        with pytest.raises(ValueError, match=f'{name}.*op-by-op path only'):
            refine_poses(m, *args, fused=True)
        assert 'fused_raygrad' not in m.__dict__
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):                   # accepted: the render is reached
        refine_poses(_model(cls, raygrad=True), *args)


def test_default_tensorf_on_the_march_refuses_such_rays_with_the_hint():
    cls = _classes()[1]
    m = _model(cls, fused_march=True)
    o, d = torch.zeros(4, 3, requires_grad=True), torch.ones(4, 3)
    with pytest.raises(NotImplementedError, match='TensoRFVoxGO has no derivative of its density with respect to the sample '
                                                  'positions: construct it with raygrad=True'):
        m.render(m.planes, o, d, d, **RK)


@pytest.mark.parametrize('which', [0, 1])
def test_rays_without_grad_and_models_without_the_option_keep_their_path(which, monkeypatch):
    """forward and render take _forward_raygrad only with the option, grad mode and rays that require grad, whatever fused
    and fused_march say, and hand it the caller's feats."""
    from directvoxgo_amd.triplane import TriPlaneVoxGO
    cls = _classes()[which]
    seen = []
    monkeypatch.setattr(cls, '_forward_raygrad', lambda self, *a, feats=None, **k: seen.append(('raygrad', feats)))
    monkeypatch.setattr(TriPlaneVoxGO, 'render', lambda self, *a, **k: seen.append(('render', None)))
    monkeypatch.setattr(cls, '_render_unfused', lambda self, *a, **k: seen.append(('render', None)))
    o, d = torch.zeros(4, 3), torch.ones(4, 3)
    og = torch.zeros(4, 3, requires_grad=True)
    more = [dict(fused_march=True)] if which == 1 else [dict()]
    for kw in [dict(), dict(fused=False)] + more:
        seen.clear()
        m = _model(cls, raygrad=True, **kw)
        m(og, d, d, **RK)
        mine = {'xy': 1}
        m.render(mine, o, d.clone().requires_grad_(), d, **RK)
        assert seen == [('raygrad', m.planes), ('raygrad', mine)], kw
    seen.clear()
    m = _model(cls, raygrad=True)
    m(o, d, d, **RK)
    with torch.no_grad():
        m(og, d, d, **RK)
    if which == 0:
        _model(cls)(og, d, d, **RK)
    else:
        _model(cls, fused=False)(og, d, d, **RK)
    assert [s[0] for s in seen] == ['render'] * 3


def test_forward_raygrad_takes_feats():
    import inspect
    from directvoxgo_amd.dvgo import DirectVoxGO
    assert inspect.signature(DirectVoxGO._forward_raygrad).parameters['feats'].default is None
