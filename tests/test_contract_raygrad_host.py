"""CPU: the contraction's ray gradient (csrc/contract_raygrad.hip) without a device.

  * tests/contract_raygrad_oracle.py equals float64 torch.autograd of a direct restatement of the contracted sample, for both
    norms and an anisotropic radius, away from n == 1 and from inf-norm ties; at constructed ties and at n == 1 exactly it
    follows the stated rules (lowest axis index; identity);
  * the kernel's arithmetic restated in float32 numpy, summed per ray in two different orders, stays inside the bound the GPU
    test applies to the kernel.  The bound is (n_ray + 32) * 2^-24 * (sum of absolute terms): 32 counts the roundings on the
    longest chain from the float32 inputs to a term of grad_d (29: contract_raygrad_oracle.ROUNDINGS derives it line by line)
    plus room for second-order terms, and the sum of a ray's n_ray terms adds at most n_ray - 1 roundings in any order;
  * host logic: `raygrad` is no get_kwargs key, the default model's refusals name the class, refine_poses(fused=True) needs
    fused_march, the header declares both entries and _lib types them, argument validation answers before any launch.
"""
import ctypes

import numpy as np
import pytest
import torch

import contract_raygrad_cases as C
import contract_raygrad_oracle as CR

NORMS_B = [('inf', 0.2), ('inf', 1.0), ('l2', 0.2), ('l2', 1.0)]
IDS = [f'{n}-b{b}' for n, b in NORMS_B]


# ---------------------------------------------------------------------------------------------- the oracle itself
def _direct64(rays_o, rays_d, center, radius, t, ray_id, b, norm):
    """q of the listed samples as a differentiable float64 function of the rays: the issue's forward, restated directly."""
    o = (rays_o - center) / radius
    u = rays_d / radius
    d = u / u.norm(dim=-1, keepdim=True)
    p = o[ray_id] + d[ray_id] * t[:, None]
    n = p.abs().amax(-1) if norm == 'inf' else p.norm(dim=-1)
    return torch.where((n <= 1)[:, None], p, p * ((1 + b) / n - b / n ** 2)[:, None]), p, n


@pytest.mark.parametrize('norm,b', NORMS_B, ids=IDS)
def test_oracle_equals_float64_autograd(norm, b):
    rng = np.random.default_rng(11)
    N, per = 40, 30
    t_tab = C.U.t_table(C.WORLD, C.STEPSIZE, b)[0].astype(np.float64)
    rays_o = rng.uniform(-2, 2, (N, 3)) * C.RADIUS + C.CENTER
    rays_d = rng.normal(size=(N, 3))
    ray_id = np.repeat(np.arange(N), per)
    step_id = np.concatenate([np.sort(rng.choice(len(t_tab), per, replace=False)) for _ in range(N)])
    g = rng.normal(size=(N * per, 3))
    b32 = float(np.float32(b))
    T = lambda x: torch.tensor(np.asarray(x, np.float64))     # noqa: E731
    o_t, d_t = T(rays_o).requires_grad_(), T(rays_d).requires_grad_()
    q, p, n = _direct64(o_t, d_t, T(C.CENTER), T(C.RADIUS), T(t_tab)[step_id], torch.tensor(ray_id), b32, norm)
    # away from the discontinuities: n == 1, and (inf) a second axis within 1e-6 of the maximum
    pa = np.sort(np.abs(p.detach().numpy()), -1)
    assert (np.abs(n.detach().numpy() - 1) > 1e-6).all() and (norm == 'l2' or (pa[:, 2] - pa[:, 1] > 1e-6).all())
    (q * T(g)).sum().backward()
    got = CR.ray_grads(rays_o, rays_d, C.CENTER, C.RADIUS, t_tab, b, norm, g, ray_id, step_id, dtype=np.float64)
    for key, ref in (('grad_o', o_t.grad.numpy()), ('grad_d', d_t.grad.numpy())):
        err = np.abs(got[key] - ref).max() / np.abs(ref).max()
        print(f'{norm} b={b} {key}: oracle vs float64 autograd, normalised max error {err:.3g}')
        assert err < 1e-12
    assert (got['abs_o'] >= np.abs(got['grad_o'])).all() and (got['abs_d'] >= np.abs(got['grad_d']) * (1 - 1e-12)).all()


def test_oracle_follows_the_tie_rule_and_n_equal_one():
    case = C.build('inf', 0.2)
    nm, rid, g = case['named'], case['ray_id'], case['g']
    o, d, _ = CR.ray_setup(case['rays_o'], case['rays_d'], C.CENTER, C.RADIUS)
    p, n, inner, axis, _ = CR.points(o, d, case['t_tab'], 0.2, 'inf', rid, case['step_id'])
    h, _ = CR._jacobian_t(p, inner, axis, 0.2, 'inf', g)
    b = float(np.float32(0.2))
    for name, ax in (('tie_xy', 0), ('tie_xy_neg', 0), ('tie_yz', 1)):
        sel = (rid == nm[name]) & ~inner
        assert sel.any() and (axis[sel] == ax).all()
        nn = np.abs(p[sel, ax]).astype(np.float64)
        f, fp = (1 + b) / nn - b / nn ** 2, -(1 + b) / nn ** 2 + 2 * b / nn ** 3
        dot = (p[sel].astype(np.float64) * g[sel]).sum(-1)
        want = f[:, None] * g[sel].astype(np.float64)
        want[:, ax] += np.sign(p[sel, ax]) * fp * dot            # the lowest tied axis alone carries the norm's derivative
        assert np.array_equal(h[sel], want)
    one = (rid == nm['n_one']) & (case['step_id'] == case['k_one'])
    assert n[one][0] == 1.0 and np.array_equal(h[one], g[one].astype(np.float64))            # n == 1 exactly: identity
    for norm in ('inf', 'l2'):                                                                # ... under both norms
        c2 = C.build(norm, 1.0)
        r = CR.ray_grads(c2['rays_o'], c2['rays_d'], C.CENTER, C.RADIUS, c2['t_tab'], 1.0, norm, c2['g'], c2['ray_id'], c2['step_id'])
        z = c2['named']['zero_g']
        assert not r['grad_o'][z].any() and not r['grad_d'][z].any() and not r['abs_d'][z].any()
        empty = np.nonzero(r['n_ray'] == 0)[0]
        assert len(empty) and not r['grad_o'][empty].any() and not r['grad_d'][empty].any()


@pytest.mark.parametrize('norm,b', NORMS_B, ids=IDS)
def test_float32_restatement_stays_inside_the_bound_in_two_orders(norm, b):
    case = C.build(norm, b)
    args = (case['rays_o'], case['rays_d'], C.CENTER, C.RADIUS, case['t_tab'], b, norm, case['g'], case['ray_id'], case['step_id'])
    ref = CR.ray_grads(*args)
    outs = {order: CR.restate_f32(*args, order=order) for order in ('lanes', 'sequential')}
    assert not all(np.array_equal(a, b_) for a, b_ in zip(outs['lanes'], outs['sequential']))      # the orders do differ
    for order, (go, gd) in outs.items():
        for key, got, ab in (('grad_o', go, ref['abs_o']), ('grad_d', gd, ref['abs_d'])):
            lim = CR.bound(ab, ref['n_ray'])
            err = np.abs(got.astype(np.float64) - ref[key])
            with np.errstate(divide='ignore', invalid='ignore'):
                worst = np.nanmax(np.where(lim > 0, err / lim, 0.0))
            print(f'{norm} b={b} {order} {key}: worst error / bound = {worst:.3f}')
            assert (err <= lim).all()
        z = case['named']['zero_g']
        assert not go[z].any() and not gd[z].any()


# ---------------------------------------------------------------------------------------------- build, typing, validation
LIST, REC = 'dvgo_contract_ray_bwd', 'dvgo_contract_ray_bwd_rec'


@pytest.fixture(scope='module')
def lib():
    from directvoxgo_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def test_header_declares_both_entries_and_lib_types_them(lib):
    from directvoxgo_amd import _lib, build
    assert 'contract_raygrad.hip' in build.SOURCES and 'contract_common.h' in build.HEADERS
    with open(_lib.HEADER_PATH) as f:
        decl = _lib.declarations(f.read())
    P, i, q, fl = _lib._Pointer, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    head = [P, P, q, P, P, P, i, fl, i]
    assert decl[LIST] == (ctypes.c_int, head + [P, P, q, P, P, P, P])
    assert decl[REC] == (ctypes.c_int, head + [P, P, q, P, P, q, P, P, P])
    for name in (LIST, REC):
        assert getattr(lib, name).argtypes == decl[name][1]
    assert _lib.ABI_VERSION == lib.dvgo_abi_version()


ONE = ctypes.c_void_p(16)         # any non-null value: rejected before it could be dereferenced, or never reached


def _host3():
    from directvoxgo_amd._lib import f3
    return f3([0.0, 0.5, 1.0])


def _list(lib, N=4, M=10, n_max=82, null=()):
    P = lambda k: None if k in null else ONE         # noqa: E731
    H = lambda k: None if k in null else _host3()    # noqa: E731  (host arrays: these are read)
    return lib.dvgo_contract_ray_bwd(P('rays_o'), P('rays_d'), N, H('center'), H('radius'), P('t_tab'), n_max, 0.2, 0, P('grad_q'),
                                     P('step_id'), M, P('off'), P('grad_o'), P('grad_d'), None)


def _rec(lib, N=4, M2=10, n_max=82, stride=82, null=()):
    P = lambda k: None if k in null else ONE         # noqa: E731
    H = lambda k: None if k in null else _host3()    # noqa: E731
    return lib.dvgo_contract_ray_bwd_rec(P('rays_o'), P('rays_d'), N, H('center'), H('radius'), P('t_tab'), n_max, 0.2, 1, P('rec2'),
                                         P('n2'), stride, P('off2'), P('grad_q2'), M2, P('grad_o'), P('grad_d'), None)


def test_validation_answers_before_any_launch(lib):
    """-1 for negative counts, n_max <= 0 or null pointers, 0 for no rays, -2 past the 32-bit launch range: none of them
    touches the device, which is what makes these calls safe on a host without a GPU."""
    need = ('rays_o', 'rays_d', 'center', 'radius', 't_tab', 'off', 'grad_o', 'grad_d')
    assert _list(lib, N=0) == 0 and _list(lib, N=0, null=need + ('grad_q', 'step_id')) == 0
    assert _list(lib, N=-1) == -1 and _list(lib, M=-1) == -1 and _list(lib, n_max=0) == -1 and _list(lib, n_max=-2) == -1
    assert _list(lib, N=0, n_max=0) == -1
    for k in need + ('grad_q', 'step_id'):
        assert _list(lib, null=(k,)) == -1, k
    assert _list(lib, N=(1 << 31) // 64) == -2
    need = ('rays_o', 'rays_d', 'center', 'radius', 't_tab', 'n2', 'off2', 'grad_o', 'grad_d')
    assert _rec(lib, N=0) == 0 and _rec(lib, N=0, null=need + ('rec2', 'grad_q2')) == 0
    assert _rec(lib, N=-1) == -1 and _rec(lib, M2=-1) == -1 and _rec(lib, n_max=0) == -1 and _rec(lib, stride=-1) == -1
    for k in need + ('rec2', 'grad_q2'):
        assert _rec(lib, null=(k,)) == -1, k
    assert _rec(lib, N=(1 << 31) // 64) == -2 and _rec(lib, stride=1 << 31) == -2
    from directvoxgo_amd import _lib
    with pytest.raises(RuntimeError, match='invalid argument'):               # the typed call turns the code into an error
        _lib.call(LIST, None, None, 4, None, None, None, 82, 0.2, 0, None, None, 0, None, None, None, None)
    with pytest.raises(TypeError, match='arguments given'):
        _lib.call(REC, None, 1, 1)


# ---------------------------------------------------------------------------------------------- model, op and pose loop, host side
def _model(**kw):
    from directvoxgo_amd.dcvgo import DirectContractedVoxGO
    args = dict(xyz_min=[-1, -2, -0.5], xyz_max=[1, 2, 1.5], num_voxels=24 ** 3, num_voxels_base=24 ** 3, alpha_init=1e-2, bg_len=0.2)
    args.update(kw)
    return DirectContractedVoxGO(**args)


RK = dict(near=0.0, far=1e4, bg=1, stepsize=0.5)


def test_raygrad_is_a_plain_attribute_and_survives_load_model(tmp_path):
    from directvoxgo_amd.checkpoint import load_model, save_checkpoint
    from directvoxgo_amd.dcvgo import DirectContractedVoxGO
    assert _model().raygrad is False and _model(raygrad=True).raygrad is True and _model(raygrad=1).raygrad is True
    m = _model(raygrad=True, fused_march=True)
    kw = m.get_kwargs()
    assert 'raygrad' not in kw and set(kw) == set(_model().get_kwargs()) and not any('raygrad' in k for k in m.state_dict())
    path = str(tmp_path / 'c.tar')
    save_checkpoint(path, m, None, 3)
    assert load_model(DirectContractedVoxGO, path).raygrad is False
    m2 = load_model(DirectContractedVoxGO, path, raygrad=True)
    assert m2.raygrad is True and m2.fused_march is False and set(m2.state_dict()) == set(m.state_dict())
    assert list(m.scene_center_h) == m.scene_center.tolist() and list(m.scene_radius_h) == m.scene_radius.tolist()
    assert m.scene_center_h is m.scene_center_h                                       # read once


def test_default_refusals_name_the_class_and_the_option():
    from directvoxgo_amd import fused as F
    o, d = torch.zeros(4, 3), torch.ones(4, 3)
    og = torch.zeros(4, 3, requires_grad=True)
    m = _model(fused_march=True)
    for rays in ((og, d), (o, d.clone().requires_grad_())):
        with pytest.raises(NotImplementedError, match='DirectContractedVoxGO.*construct it with raygrad=True'):
            m(*rays, d, **RK)
    cfg = m._march_contract_cfg(0.5, 'cpu')
    with pytest.raises(NotImplementedError, match='fused_march_contract.*require grad'):
        F.fused_march_contract(m.density, og, d, cfg)
    with pytest.raises(NotImplementedError, match='fused_march_contract.*require grad'):
        F.fused_march_contract(m.density, og, d, cfg, raygrad=False)
    for mm in (_model(raygrad=True, fused_march=True), _model(raygrad=True)):         # with the option the rays reach the kernels,
        with pytest.raises(RuntimeError, match='must be a CUDA tensor'):               # which have no CPU fallback
            mm(og, d, d, **RK)
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        F.fused_march_contract(m.density, og, d, cfg, raygrad=True)
    with torch.no_grad():                                                              # without grad mode nothing changes
        with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
            _model(raygrad=True, fused_march=True)(og, d, d, **RK)


def test_contract_points_checks_its_inputs():
    from directvoxgo_amd.ops import contract_points
    o, d = torch.zeros(2, 3), torch.ones(2, 3)
    rid, sid, q, t = torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int64), torch.zeros(3, 3), torch.ones(5)
    with pytest.raises(ValueError, match='contracted_norm'):
        contract_points(o, d, rid, sid, q, [0, 0, 0], [1, 1, 1], t, 0.2, 'l1')
    with pytest.raises(RuntimeError, match='rays_o must be a CUDA tensor'):
        contract_points(o, d, rid, sid, q, [0, 0, 0], [1, 1, 1], t, 0.2, 'inf')


def test_refine_poses_accepts_only_the_model_with_raygrad():
    from directvoxgo_amd.pose import CameraRefiner, _supported, refine_poses
    from directvoxgo_amd.train import FINE_TRAIN
    H = W = 4
    K = [[4.0, 0, 2], [0, 4.0, 2], [0, 0, 1]]
    ref = CameraRefiner(np.eye(4, dtype=np.float32)[None, :3], [[H, W]], [K])
    args = (ref, torch.zeros(1, H, W, 3), FINE_TRAIN, RK, 1, 8, 1e-3)
    assert not _supported(_model()) and not _supported(_model(fused_march=True))
    assert _supported(_model(raygrad=True)) and _supported(_model(raygrad=True, fused_march=True))
    with pytest.raises(NotImplementedError, match='DirectContractedVoxGO.*construct it with raygrad=True'):
        refine_poses(_model(), *args)
    with pytest.raises(ValueError, match='fused_march'):
        refine_poses(_model(raygrad=True), *args, fused=True)
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):                   # accepted: the render is reached
        refine_poses(_model(raygrad=True), *args)
