"""GPU: ray gradients through the scene contraction (csrc/contract_raygrad.hip, ops.contract_points,
DirectContractedVoxGO(raygrad=True), pose.refine_poses on unbounded scenes).

 1. both kernel entries against tests/contract_raygrad_oracle.py on the hand-built rays of tests/contract_raygrad_cases.py:
    every element inside (n_ray + 32) * 2^-24 * sum|terms| (the oracle module derives the 32), two launches bit-equal, the
    record entry bit-equal to the list entry;
 2. with raygrad=True and rays that require grad, every result key has the bits of the raygrad=False forward, on both paths;
 3. stage by stage: dL/dq captured at the wrapped positions (and, on the fused march, the per-record g_q2 handed to the
    record entry) fed to the oracle bounds the model's rays_o.grad / rays_d.grad; a frozen model gives the same bits;
 4. end to end against float64 torch.autograd of tests/contract_render_oracle.py with the kept set fixed.  This tolerance
    cannot be derived: the yardstick is the same restatement run in float32 torch ops, and 4x its error is allowed (the
    kernels sum in different but equally valid orders across three float32 stages);
 5. fused march against op by op: the ray gradients agree, relative to the sum of absolute terms, within 8x the
    disagreement of the two paths' density.grad on the same scene (two more float32 stages), measured in the same test;
 6. refine_poses recovers perturbed poses of an unbounded capture on both paths, and moves poses and model together.

Measured values are printed (run with -s) and recorded in profiles/contract_raygrad/README.md.
"""
import math

import numpy as np
import pytest
import torch

import contract_raygrad_cases as C
import contract_raygrad_oracle as CR
import contract_render_oracle as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- 1. kernel vs oracle
def _launch_list(case, g=None):
    from directvoxgo_amd import _lib as L
    o, d = _cuda(case['rays_o']), _cuda(case['rays_d'])
    N = o.shape[0]
    go = torch.full((N, 3), 7.0, device=DEV)                   # (nothing to zero beforehand: every row is written)
    gd = torch.full((N, 3), 7.0, device=DEV)
    g = _cuda(case['g'] if g is None else g)
    L.call('dvgo_contract_ray_bwd', o, d, N, L.f3(C.CENTER), L.f3(C.RADIUS), _cuda(case['t_tab']), case['n_max'], float(case['b']),
           1 if case['norm'] == 'l2' else 0, g, _cuda(case['step_id']), g.shape[0], _cuda(case['off']), go, gd, L.stream_of(o))
    return go.cpu().numpy(), gd.cpu().numpy()


def _launch_rec(case):
    from directvoxgo_amd import _lib as L
    o, d = _cuda(case['rays_o']), _cuda(case['rays_d'])
    N = o.shape[0]
    rec, n2 = C.records(case)
    go, gd = torch.full((N, 3), 7.0, device=DEV), torch.full((N, 3), 7.0, device=DEV)
    g = _cuda(case['g'])
    L.call('dvgo_contract_ray_bwd_rec', o, d, N, L.f3(C.CENTER), L.f3(C.RADIUS), _cuda(case['t_tab']), case['n_max'], float(case['b']),
           1 if case['norm'] == 'l2' else 0, _cuda(rec), _cuda(n2), C.REC_STRIDE, _cuda(case['off']), g, g.shape[0], go, gd,
           L.stream_of(o))
    return go.cpu().numpy(), gd.cpu().numpy()


@pytest.mark.parametrize('norm,b', [('inf', 0.2), ('inf', 1.0), ('l2', 0.2), ('l2', 1.0)])
def test_both_entries_match_the_oracle_inside_the_derived_bound(norm, b):
    case = C.build(norm, b)
    assert case['n_max'] == (82 if b == 0.2 else 50) and case['rays_o'].shape[0] == 48
    ref = CR.ray_grads(case['rays_o'], case['rays_d'], C.CENTER, C.RADIUS, case['t_tab'], b, norm, case['g'], case['ray_id'],
                       case['step_id'])
    go, gd = _launch_list(case)
    assert np.isfinite(go).all() and np.isfinite(gd).all()
    for key, got, ab in (('grad_o', go, ref['abs_o']), ('grad_d', gd, ref['abs_d'])):
        lim = CR.bound(ab, ref['n_ray'])
        err = np.abs(got.astype(np.float64) - ref[key])
        with np.errstate(divide='ignore', invalid='ignore'):
            worst = np.nanmax(np.where(lim > 0, err / lim, 0.0))
        print(f'\ncontract_ray_bwd {norm} b={b} {key}: worst error / bound = {worst:.3f}, max |ref| {np.abs(ref[key]).max():.4g}', end='')
        assert (err <= lim).all(), (key, worst)                 # every element, none excluded
        assert np.abs(ref[key]).max() > 1
    empty = np.nonzero(ref['n_ray'] == 0)[0]
    z = case['named']['zero_g']
    for rows in (empty, [z]):                                   # exact zeros: a ray without samples, a ray whose grad_q is zero
        assert len(rows) and not go[rows].any() and not gd[rows].any()
    go2, gd2 = _launch_list(case)
    assert np.array_equal(go.view(np.int32), go2.view(np.int32)) and np.array_equal(gd.view(np.int32), gd2.view(np.int32))
    gor, gdr = _launch_rec(case)                                # the same samples as records: the same bits
    assert np.array_equal(go.view(np.int32), gor.view(np.int32)) and np.array_equal(gd.view(np.int32), gdr.view(np.int32))


def test_a_step_outside_the_table_marks_its_ray_and_reads_nothing():
    case = C.build('inf', 0.2)
    go, gd = _launch_list(case)
    bad = dict(case, step_id=case['step_id'].copy())
    r = case['named']['outside']
    a = case['off'][r]
    bad['step_id'][a + 3] = case['n_max']                       # one past the table
    bad['step_id'][a + 70] = -1
    go2, gd2 = _launch_list(bad)
    assert np.isnan(go2[r]).all() and np.isnan(gd2[r]).all()
    others = np.arange(go.shape[0]) != r
    assert np.array_equal(go[others].view(np.int32), go2[others].view(np.int32))
    assert np.array_equal(gd[others].view(np.int32), gd2[others].view(np.int32))


# ---------------------------------------------------------------------------------------------- the scene of 2. to 5.
@pytest.fixture(scope='module')
def scene():
    from directvoxgo_amd import scenes
    sc = scenes.unbounded_scene(world=24, H=8, W=8)
    for p in sc['gt'].parameters():
        p.requires_grad_(False)
    return sc


def _model(scene, fused_march, raygrad, thres=0, frozen=False):
    from directvoxgo_amd.dcvgo import DirectContractedVoxGO
    gt = scene['gt']
    kw = gt.get_kwargs()
    kw.pop('act_shift'), kw.pop('voxel_size_ratio')
    kw['fast_color_thres'] = thres
    m = DirectContractedVoxGO(**kw, fused_march=fused_march, raygrad=raygrad).to(DEV)
    m.load_state_dict(gt.state_dict())
    for p in m.parameters():
        p.requires_grad_(not frozen)
    return m


def _rays(scene, n=192, grad=True):
    """Every 8th ray of the training views: inward and outward cameras, blob, shell and empty space."""
    sel = slice(0, 8 * n, 8)
    o, d, v = (scene[k][sel].clone() for k in ('rays_o', 'rays_d', 'viewdirs'))
    if grad:
        o.requires_grad_(), d.requires_grad_()
    return o, d, v


def _loss(res, G, n_rays):
    from directvoxgo_amd.train import distortion_term
    return (res['rgb_marched'] * G).sum() + distortion_term(res, n_rays, {'weight_distortion': 0.01})


@pytest.fixture(scope='module')
def G(scene):
    gen = torch.Generator().manual_seed(3)
    return torch.randn((192, 3), generator=gen).to(DEV)


# ---------------------------------------------------------------------------------------------- 2. forward bits
@pytest.mark.parametrize('thres', [0, 1e-4])
@pytest.mark.parametrize('fused_march', [False, True], ids=['op-by-op', 'fused-march'])
def test_forward_bits_are_those_of_the_forward_without_raygrad(scene, fused_march, thres):
    rk = dict(scene['render_kwargs'], render_depth=True)
    o, d, v = _rays(scene, grad=False)
    with torch.no_grad():
        want = _model(scene, fused_march, False, thres)(o, d, v, **rk)
    og, dg, _ = _rays(scene)
    got = _model(scene, fused_march, True, thres)(og, dg, v, **rk)
    assert got['rgb_marched'].requires_grad and set(got) == set(want)
    assert got['weights'].shape[0] > 1000
    for k, w in want.items():
        if isinstance(w, torch.Tensor):
            assert same_bits(got[k].detach(), w), k
        else:
            assert got[k] == w, k


# ---------------------------------------------------------------------------------------------- 3. stagewise chain
class _Capture:
    """Records what the model hands to the ray-gradient kernels: dL/dq at the wrapped positions (a tensor hook) and, on the
    fused march, the record entry's arguments."""

    def __init__(self, monkeypatch):
        from directvoxgo_amd import _lib, dcvgo
        self.wrapped, self.rec = [], []
        real_cp, real_call = dcvgo.contract_points, _lib.call

        def cp(rays_o, rays_d, ray_id, step_id, q, *rest):
            out = real_cp(rays_o, rays_d, ray_id, step_id, q, *rest)
            entry = dict(ray_id=ray_id, step_id=step_id)
            out.register_hook(lambda g: entry.__setitem__('g', g.detach().clone()))
            self.wrapped.append(entry)
            return out

        def call(name, *args):
            if name == 'dvgo_contract_ray_bwd_rec':
                rec2, n2, stride, off2, g_q2 = args[9:14]
                self.rec.append(dict(rec2=rec2.clone(), n2=n2.clone(), stride=stride, g=g_q2.clone()))
            return real_call(name, *args)

        monkeypatch.setattr(dcvgo, 'contract_points', cp)
        monkeypatch.setattr(_lib, 'call', call)

    def lists(self):
        """-> [(ray_id, step_id, g)] numpy: the wrapped positions' list, then (fused march) the records as a list."""
        out = [(e['ray_id'].cpu().numpy(), e['step_id'].cpu().numpy(), e['g'].cpu().numpy()) for e in self.wrapped]
        for e in self.rec:
            n2 = e['n2'].cpu().numpy()
            step = e['rec2'].view(torch.int32)[:, 0].cpu().numpy().reshape(len(n2), e['stride'])
            rid = np.repeat(np.arange(len(n2)), n2)
            sid = np.concatenate([step[r, :n2[r]] & 0x7fffffff for r in range(len(n2))]).astype(np.int64)
            out.append((rid, sid, e['g'].cpu().numpy()))
        return out


def _oracle_sum(model, o, d, t_tab, lists):
    """float64 ray gradients and their bound from the captured per-sample gradients.  Each list is one kernel launch, inside
    its own bound; autograd's addition of the launches' results is one more rounding of a sum that the absolute terms bound."""
    c, r = model.scene_center.cpu().numpy(), model.scene_radius.cpu().numpy()
    tot = {k: 0.0 for k in ('grad_o', 'grad_d', 'abs_o', 'abs_d', 'lim_o', 'lim_d')}
    for rid, sid, g in lists:
        ref = CR.ray_grads(o, d, c, r, t_tab, model.bg_len, model.contracted_norm, g, rid, sid)
        for k in ('grad_o', 'grad_d', 'abs_o', 'abs_d'):
            tot[k] = tot[k] + ref[k]
        tot['lim_o'] = tot['lim_o'] + CR.bound(ref['abs_o'], ref['n_ray'])
        tot['lim_d'] = tot['lim_d'] + CR.bound(ref['abs_d'], ref['n_ray'])
    if len(lists) > 1:
        tot['lim_o'] = tot['lim_o'] + CR.EPS * tot['abs_o']
        tot['lim_d'] = tot['lim_d'] + CR.EPS * tot['abs_d']
    return tot


def _backward(model, scene, G, monkeypatch=None):
    cap = _Capture(monkeypatch) if monkeypatch is not None else None
    o, d, v = _rays(scene)
    res = model(o, d, v, **scene['render_kwargs'])
    _loss(res, G, o.shape[0]).backward()
    return o, d, res, cap


@pytest.mark.parametrize('thres', [0, 1e-4])
@pytest.mark.parametrize('fused_march', [False, True], ids=['op-by-op', 'fused-march'])
def test_ray_gradients_follow_the_oracle_stage_by_stage(scene, G, monkeypatch, fused_march, thres):
    m = _model(scene, fused_march, True, thres)
    o, d, res, cap = _backward(m, scene, G, monkeypatch)
    monkeypatch.undo()
    assert len(cap.wrapped) == 1 and len(cap.rec) == (1 if fused_march else 0)
    t_tab = m._table(scene['render_kwargs']['stepsize'], DEV)[0].cpu().numpy()
    ref = _oracle_sum(m, o.detach().cpu().numpy(), d.detach().cpu().numpy(), t_tab, cap.lists())
    for key, got, lim in (('grad_o', o.grad, ref['lim_o']), ('grad_d', d.grad, ref['lim_d'])):
        err = np.abs(got.cpu().numpy().astype(np.float64) - ref[key])
        with np.errstate(divide='ignore', invalid='ignore'):
            worst = np.nanmax(np.where(lim > 0, err / lim, 0.0))
        print(f'\nstagewise {"fused" if fused_march else "op-by-op"} thres={thres} {key}: worst error / bound = {worst:.3f}, '
              f'max |ref| {np.abs(ref[key]).max():.4g}', end='')
        assert np.abs(ref[key]).max() > 1e-3 and (err <= lim).all(), (key, worst)
    assert m.density.grad is not None and m.k0.grad is not None
    # a frozen model: the same ray gradients, and its parameters are left alone
    fz = _model(scene, fused_march, True, thres, frozen=True)
    o2, d2, _, _ = _backward(fz, scene, G)
    assert same_bits(o2.grad, o.grad) and same_bits(d2.grad, d.grad)
    assert all(p.grad is None for p in fz.parameters())


# ---------------------------------------------------------------------------------------------- 4. end to end against float64
def _restated_grads(model, scene, G, kept, dtype):
    o, d, _ = _rays(scene, grad=False)
    o, d = o.cpu().to(dtype).requires_grad_(), d.cpu().to(dtype).requires_grad_()
    T = lambda x: torch.as_tensor(x).detach().cpu().to(dtype)     # noqa: E731
    rid, sid = kept
    t_tab = T(model._table(scene['render_kwargs']['stepsize'], DEV)[0])
    b = float(np.float32(model.bg_len))
    res = R.render(o, d, rid, sid, t_tab, T(model.scene_center), T(model.scene_radius), b, model.contracted_norm,
                   T(model.density)[0, 0], T(model.k0)[0], float(model.act_shift),
                   float(scene['render_kwargs']['stepsize'] * model.voxel_size_ratio), scene['render_kwargs']['bg'])
    loss = (res['rgb_marched'] * T(G)).sum() + 0.01 * R.distortion(res['weights'], rid, sid, t_tab, o.shape[0])
    loss.backward()
    return o.grad.double(), d.grad.double(), res


def test_end_to_end_against_float64_autograd(scene, G):
    """Measured on an MI355X (normalised max error against the float64 gradient; see profiles/contract_raygrad/README.md):
    the values are printed below and recorded there."""
    out = {}
    for name, fused_march in (('op-by-op', False), ('fused-march', True)):
        m = _model(scene, fused_march, True)
        o, d, res, _ = _backward(m, scene, G)
        out[name] = (o.grad.cpu().double(), d.grad.cpu().double(), res)
    # the kept set, fixed: the fused march's (with fast_color_thres == 0 the op-by-op list also carries the samples behind a
    # ray's stop, with weight exactly 0 and no gradient)
    res_f = out['fused-march'][2]
    kept = (res_f['ray_id'].cpu(), res_f['step_id'].cpu())
    o64, d64, r64 = _restated_grads(m, scene, G, kept, torch.float64)
    o32, d32, _ = _restated_grads(m, scene, G, kept, torch.float32)
    assert float((r64['rgb_marched'].detach() - res_f['rgb_marched'].detach().cpu().double()).abs().max()) < 1e-4   # the restatement is this render
    for what, g64, g32, i in (('rays_o.grad', o64, o32, 0), ('rays_d.grad', d64, d32, 1)):
        scale = float(g64.abs().max())
        e32 = float((g32 - g64).abs().max()) / scale
        assert scale > 1e-3 and e32 > 0
        for name in out:
            err = float((out[name][i] - g64).abs().max()) / scale
            print(f'\nend to end {name} {what}: max |g64| {scale:.4g}  float32 torch ops {e32:.4g}  kernels {err:.4g}  (allowed {4 * e32:.4g})', end='')
            assert err <= 4 * e32, (name, what, err, e32)


# ---------------------------------------------------------------------------------------------- 5. fused vs op by op
def test_fused_march_and_op_by_op_agree(scene, G, monkeypatch):
    from directvoxgo_amd import ops
    mu, mf = _model(scene, False, True), _model(scene, True, True)
    ou, du, _, cap = _backward(mu, scene, G, monkeypatch)
    monkeypatch.undo()
    of, df, _, _ = _backward(mf, scene, G)
    # the sums of absolute terms: of the ray gradients from the oracle on the captured dL/dq ...
    t_tab = mu._table(scene['render_kwargs']['stepsize'], DEV)[0].cpu().numpy()
    ref = _oracle_sum(mu, ou.detach().cpu().numpy(), du.detach().cpu().numpy(), t_tab, cap.lists())
    # ... and of density.grad: the scatter is linear in the per-sample raw-density gradient with weights >= 0, so the scatter
    # of its absolute values is the sum of absolute terms.  dL/draw = the density sample's gradient, captured by a hook
    seen = {}
    o, d, v = _rays(scene)
    real = mu.grid_sampler

    def sampler(xyz, grid):
        out = real(xyz, grid)
        if grid is mu.density:
            seen['q'] = xyz.detach()
            out.register_hook(lambda g: seen.__setitem__('g', g.detach().clone()))
        return out

    monkeypatch.setattr(mu, 'grid_sampler', sampler)
    mu.zero_grad()
    _loss(mu(o, d, v, **scene['render_kwargs']), G, o.shape[0]).backward()
    monkeypatch.undo()
    leaf = mu.density.detach().clone().requires_grad_()
    ops.grid_sample(leaf, seen['q'], mu.xyz_min, mu.xyz_max).backward(seen['g'].abs())
    abs_density = float(leaf.grad.max())
    e_density = float((mu.density.grad - mf.density.grad).abs().max()) / abs_density
    e_o = float((ou.grad - of.grad).abs().max()) / float(ref['abs_o'].max())
    e_d = float((du.grad - df.grad).abs().max()) / float(ref['abs_d'].max())
    print(f'\nfused march vs op by op, relative to the largest sum of absolute terms: density.grad {e_density:.4g}  '
          f'rays_o.grad {e_o:.4g}  rays_d.grad {e_d:.4g}  (allowed {8 * e_density:.4g})', end='')
    assert e_density > 0
    assert e_o <= 8 * e_density and e_d <= 8 * e_density


# ---------------------------------------------------------------------------------------------- 6. recovery
# The capture: scenes.unbounded_scene(world=32, 6 views of 16 x 16, focal 12), every pose turned by 1 degree about a random axis
# and moved by 0.03 (the cameras sit 0.55 .. 0.85 from the origin of a foreground box of half-size 1).  Adam moves a parameter
# by about the step size per iteration while its gradient keeps its sign; a view needs up to 0.85 * 0.0175 + 0.03 = 0.045 in
# delta's units, i.e. 45 iterations at 1e-3, which leaves three quarters of the 200 to settle.  Checked on the CPU
# (tools/contract_raygrad_descent_cpu.py, its defaults): Adam at lrate 1e-3 on float64 torch.autograd of
# tests/contract_render_oracle.py (targets from the same restatement at the true poses, the kept set from
# tests/unbounded_oracle.py's sampler) descends from this start, loss 1.5e-3 -> 3.1e-5 in 200 iterations,
# every view's rotation error from 1 degree to at most 0.40 and every translation error from 0.03 to at most 0.015.
ROT_DEG, SHIFT, LRATE_POSE = 1.0, 0.03, 1e-3


@pytest.fixture(scope='module')
def capture():
    from directvoxgo_amd import scenes
    from directvoxgo_amd.pose import se3_exp
    sc = scenes.unbounded_scene(world=32, n_train=6, n_test=0, H=16, W=16, focal=12.0)
    true = torch.from_numpy(sc['train_poses'])[:, :3, :4].float()
    n = true.shape[0]
    gen = torch.Generator().manual_seed(7)
    axis = torch.randn(n, 3, generator=gen)
    axis = axis / axis.norm(dim=-1, keepdim=True)
    shift = torch.randn(n, 3, generator=gen)
    shift = shift / shift.norm(dim=-1, keepdim=True) * SHIFT
    E = se3_exp(torch.cat([axis * math.radians(ROT_DEG), torch.zeros(n, 3)], -1))[:, :, :3]
    noisy = torch.cat([E @ true[:, :, :3], true[:, :, 3:] + shift[:, :, None]], -1)
    K = np.array([[12.0, 0, 8], [0, 12.0, 8], [0, 0, 1]], np.float32)
    images = sc['target'].reshape(n, 16, 16, 3)
    assert float(images.std()) > 0.05                            # there is something to register against
    return dict(sc=sc, true=true, noisy=noisy, HW=np.array([[16, 16]] * n), Ks=np.stack([K] * n), images=images)


def _pose_errors(est, true):
    est, true = est.detach().cpu().double(), true.cpu().double()
    rel = est[:, :, :3] @ true[:, :, :3].transpose(1, 2)
    cos = ((rel.diagonal(dim1=1, dim2=2).sum(-1) - 1) / 2).clamp(-1, 1)
    return torch.acos(cos), (est[:, :, 3] - true[:, :, 3]).norm(dim=-1)


@pytest.mark.parametrize('fused_march', [False, True], ids=['op-by-op', 'fused-march'])
def test_refine_poses_recovers_a_perturbed_unbounded_capture(capture, fused_march):
    from directvoxgo_amd.pose import CameraRefiner, refine_poses
    from directvoxgo_amd.train import COARSE_TRAIN
    c = capture
    rk = c['sc']['render_kwargs']
    m = _model(c['sc'], fused_march, True, frozen=True)
    ref = CameraRefiner(c['noisy'], c['HW'], c['Ks']).to(DEV)
    rot0, tr0 = _pose_errors(ref.poses(), c['true'])
    assert torch.allclose(rot0, torch.full_like(rot0, math.radians(ROT_DEG)), atol=1e-4) and torch.allclose(tr0, torch.full_like(tr0, SHIFT), atol=1e-4)
    cfg = dict(COARSE_TRAIN, weight_entropy_last=0.0, weight_rgbper=0.0)
    losses = refine_poses(m, ref, c['images'], cfg, rk, n_iters=200, n_rand=None, lrate_pose=LRATE_POSE, fused=fused_march)
    rot1, tr1 = _pose_errors(ref.poses(), c['true'])
    print(f'\nrefine_poses {"fused march" if fused_march else "op by op"}: loss {losses[0]:.3e} -> {losses[-1]:.3e}; rotation error (deg) '
          f'{np.degrees(rot0.numpy()).round(3).tolist()} -> {np.degrees(rot1.numpy()).round(3).tolist()}; translation error '
          f'{tr0.numpy().round(4).tolist()} -> {tr1.numpy().round(4).tolist()}', end='')
    assert len(losses) == 200 and all(math.isfinite(x) for x in losses)
    assert losses[-1] < losses[0]
    assert bool((rot1 < rot0).all()) and bool((tr1 < tr0).all())
    assert all(q.grad is None for q in m.parameters())          # a frozen model is left alone


@pytest.mark.parametrize('fused', [False, True], ids=['second-optimiser', 'train-step'])
def test_refine_poses_moves_poses_and_model_together(capture, fused):
    from directvoxgo_amd.pose import CameraRefiner, refine_poses
    from directvoxgo_amd.train import COARSE_TRAIN
    c = capture
    m = _model(c['sc'], fused, True)
    ref = CameraRefiner(c['noisy'], c['HW'], c['Ks']).to(DEV)
    before = (m.density.detach().clone(), m.k0.detach().clone())
    cfg = dict(COARSE_TRAIN, weight_distortion=0.01)
    losses = refine_poses(m, ref, c['images'], cfg, c['sc']['render_kwargs'], n_iters=20, n_rand=1024, lrate_pose=LRATE_POSE,
                          train_model=True, seed=1, fused=fused)
    assert len(losses) == 20 and all(math.isfinite(x) for x in losses)
    for g in (m.density.grad, m.k0.grad, ref.delta.grad):
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().sum()) > 0
    assert not torch.equal(before[0], m.density.detach()) and not torch.equal(before[1], m.k0.detach())
    assert bool(torch.isfinite(ref.delta).all()) and float(ref.delta.detach().abs().sum()) > 0
