"""GPU: the fused march over contracted space (csrc/march_contract.hip), `fused.fused_march_contract` and
`DirectContractedVoxGO(fused_march=True)`.

  1. the edge-case table (tests/march_contract_cases.py) through the entry point itself: the records equal, bit for bit, what
     tests/unbounded_oracle.sample followed by the filters leaves (the alphas of the candidates from dvgo_grid_sample_fwd and
     dvgo_raw2alpha, the float32 transmittance recurrence restated in numpy); tests/march_oracle.py's exact statements on the
     records; ray_id, step_id, q, t of the kept samples array_equal to the oracle's; exp_d / alpha of every record equal
     dvgo_raw2alpha of dvgo_grid_sample_fwd at the record's position; every case hits its edge; two launches byte for byte;
  2. the model: both paths from one state dict give equal tensors in every key, over the table and on the synthetic
     unbounded scene.  With fast_color_thres == 0 the op-by-op path also lists the samples behind a ray's stop, with weight
     exactly 0; the march never visits them (as DirectVoxGO's fused march does not): there the per-sample keys are equal on
     the march's samples, which must be all of the op-by-op samples but zero-weight ones, and the per-ray keys are equal;
  3. the backward kernel against `march_oracle.density_bwd_reference(order='tree')`, every record, the derived bound and the
     zero rule; q2 bit-equal to the positions; rays of 1, 63, 64, 65 and 129 records;
  4. density, k0 and colour-head gradients of the fused path against float64 with the tolerances of
     tests/test_gpu_unbounded.py::test_forward_and_grads_match_float64; one TrainStep with the distortion loss on each path;
  5. what the fused forward launches, its one host read, the fallback above the scratch budget, scale_volume_grid, a
     checkpoint round trip and the refusal of rays that require grad.
No bound here was fitted to this kernel.
"""
import contextlib

import numpy as np
import pytest
import torch

import march_contract_cases as K
import march_oracle as M
import unbounded_oracle as U

pytestmark = pytest.mark.gpu

CASES = K.cases()
IDS = [c.name for c in CASES]
RESULT_KEYS = {'alphainv_last', 'weights', 'rgb_marched', 'raw_alpha', 'raw_rgb', 'ray_id', 'step_id', 't', 's', 'n_max', 'depth'}


def _cuda(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda', dtype=dtype)


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class _Spy(contextlib.AbstractContextManager):
    """records (name, args) of every library call issued inside"""

    def __enter__(self):
        from directvoxgo_amd import _lib as L
        self._L, self._orig, self.calls = L, L.call, []
        L.call = lambda name, *args: (self.calls.append((name, args)), self._orig(name, *args))[1]
        return self

    def __exit__(self, *exc):
        self._L.call = self._orig
        return False

    def names(self):
        return [n for n, _ in self.calls]


def _case_cfg(c):
    from directvoxgo_amd import fused as F
    kw = {}
    if c.mask is not None:
        kw = dict(mask=_cuda(c.mask, torch.bool), xyz2ijk_scale=_cuda(c.mask_scale), xyz2ijk_shift=_cuda(c.mask_shift))
    return F.ContractMarchConfig(_cuda(c.center), _cuda(c.radius), _cuda(c.t_tab), c.b, c.norm, float(c.thin), _cuda(c.xyz_min),
                                 _cuda(c.xyz_max), c.act_shift, c.interval, c.thres, **kw)


class _Launch:
    """One dvgo_march_contract_density through `_lib.call` -> the device's outputs and the `Records` of them."""

    def __init__(self, c, cfg=None):
        from directvoxgo_amd import _lib as L
        self.c, self.cfg = c, cfg or _case_cfg(c)
        cfg = self.cfg
        self.o, self.d = _cuda(c.rays_o), _cuda(c.rays_d)
        self.density = _cuda(c.density)[None, None]
        N, W = c.N, c.world
        self.N, self.stride = N, cfg.n_max
        dev = self.o.device
        self.n2, self.n3 = torch.zeros(N, dtype=torch.int32, device=dev), torch.zeros(N, dtype=torch.int32, device=dev)
        self.last = torch.zeros(N, device=dev)
        self.rec2 = torch.zeros((self.stride * N, 4), device=dev)
        m = cfg.mask
        ms = m.shape if m is not None else (0, 0, 0)
        self.head = (self.o, self.d, N, cfg.center_h, cfg.radius_h, cfg.t_tab, cfg.n_max, cfg.bg_len, cfg.l2)
        L.call('dvgo_march_contract_density', *self.head, cfg.thin_thres, m, ms[0], ms[1], ms[2], cfg.scale_h, cfg.shift_h,
               self.density, W, W, W, cfg.xyz_min_h, cfg.xyz_max_h, cfg.act_shift, cfg.interval, cfg.thres, self.stride, self.rec2,
               self.n2, self.n3, self.last, L.stream_of(self.o))
        torch.cuda.synchronize()
        self.R = M.Records(_np(self.rec2), _np(self.n2), np.arange(N, dtype=np.int64) * self.stride)
        self.off3 = torch.zeros(N + 1, dtype=torch.int64, device=dev)
        self.off3[1:] = torch.cumsum(self.n3, 0)
        self.off2 = torch.zeros(N + 1, dtype=torch.int64, device=dev)
        self.off2[1:] = torch.cumsum(self.n2, 0)

    def outputs(self):
        return (self.rec2, self.n2, self.n3, self.last)

    def positions(self, ray, step):
        """dvgo_contract_positions of (ray, step) pairs -> q [M,3], t [M]"""
        from directvoxgo_amd import _lib as L
        ray, step = _cuda(ray, torch.int64), _cuda(step, torch.int64)
        Mn = ray.shape[0]
        q, t = torch.full((Mn, 3), float('nan'), device='cuda'), torch.full((Mn,), float('nan'), device='cuda')
        L.call('dvgo_contract_positions', *self.head, ray, step, Mn, q, t, L.stream_of(q))
        torch.cuda.synchronize()
        return q, t

    def gather(self):
        from directvoxgo_amd import _lib as L
        M3 = int(self.off3[-1])
        dev = self.rec2.device
        ray_id, step_id = torch.zeros(M3, dtype=torch.int64, device=dev), torch.zeros(M3, dtype=torch.int64, device=dev)
        w, a = torch.zeros(M3, device=dev), torch.zeros(M3, device=dev)
        cfg = self.cfg
        L.call('dvgo_march_gather', self.rec2, self.n2, self.off3, None, self.stride, self.off3, self.N, M3, self.o, self.d, 1.0,
               cfg.xyz_min_h, cfg.xyz_max_h, None, 0, 1, 1, 1, 1, 1, 1, 1, ray_id, step_id, w, a, None, L.stream_of(w))
        torch.cuda.synchronize()
        return ray_id, step_id, w, a

    def backward(self, gw, gl):
        """dvgo_march_contract_density_bwd -> (g_raw [M2], q2 [M2, 3])"""
        from directvoxgo_amd import _lib as L
        M2 = int(self.off2[-1])
        dev = self.rec2.device
        g_raw, q2 = torch.full((M2,), float('nan'), device=dev), torch.full((M2, 3), float('nan'), device=dev)
        cfg = self.cfg
        L.call('dvgo_march_contract_density_bwd', self.rec2, self.n2, self.stride, self.off3, self.off2, self.N, self.o, self.d,
               cfg.center_h, cfg.radius_h, cfg.t_tab, cfg.n_max, cfg.bg_len, cfg.l2, self.last, cfg.interval, gw, gl, g_raw, q2,
               L.stream_of(g_raw))
        torch.cuda.synchronize()
        return g_raw, q2

    def alpha_at(self, q):
        """(exp_d, alpha) of dvgo_raw2alpha of dvgo_grid_sample_fwd at positions q [M,3] (device tensors)"""
        from directvoxgo_amd import render_utils
        from directvoxgo_amd.ops import grid_sample
        raw = grid_sample(self.density, q, self.cfg.xyz_min_t, self.cfg.xyz_max_t).reshape(-1).contiguous()
        return render_utils.raw2alpha(raw, self.cfg.act_shift, self.cfg.interval)


@pytest.fixture(scope='module')
def launches(oracle):
    """every case launched once, with the oracle's candidates: shared by the tests below and left unchanged"""
    out = {}
    for c in CASES:
        out[c.name] = (_Launch(c), c.candidates())
    return out


# ------------------------------------------------------------------------------------------ 1. kept set and records
@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_kept_set_and_records(c, launches):
    q, (cq, cray, cstep, ct) = launches[c.name]
    N, R = c.N, q.R
    # the reference: the oracle's candidates, their alphas from the library's own sampler and activation, then the filters
    e_c, a_c = (_np(x) for x in q.alpha_at(_cuda(cq))) if cq.shape[0] else (np.zeros(0, np.float32),) * 2
    assert np.isfinite(e_c).all() and np.isfinite(a_c).all()
    rec, flag, T, last = K.march_filters(a_c, cray, N, c.thres)
    E = int(rec.sum())
    assert R.ray.shape[0] == E and np.array_equal(_np(q.n2), np.bincount(cray[rec], minlength=N))       # no record left out
    assert np.array_equal(R.ray, cray[rec]) and np.array_equal(R.step, cstep[rec]) and np.array_equal(R.flag, flag[rec])
    assert np.array_equal(_bits(R.alpha), _bits(a_c[rec])) and np.array_equal(_bits(R.exp_d), _bits(e_c[rec]))
    assert np.array_equal(_bits(R.T), _bits(T[rec])) and np.array_equal(_bits(_np(q.last)), _bits(last))
    assert np.array_equal(_np(q.n3), np.bincount(cray[flag], minlength=N))
    # march_oracle's exact statements on the device's records
    assert M.check_records(R, np.full(N, c.n_max, np.int64), c.thres, _np(q.n3), _np(q.last)) == E
    # the kept samples
    ray_id, step_id, w, a = q.gather()
    M3 = int(q.off3[-1])
    assert M.check_gather(R, _np(q.n3), _np(q.off3), _np(ray_id), _np(step_id), _np(w), _np(a)) == M3 == int(flag.sum())
    qd, td = q.positions(_np(ray_id), _np(step_id))
    assert np.array_equal(_np(ray_id), cray[flag]) and np.array_equal(_np(step_id), cstep[flag])
    assert np.array_equal(_bits(_np(qd)), _bits(cq[flag])) and np.array_equal(_bits(_np(td)), _bits(ct[flag]))
    # the bits of the density, at the positions the library itself gives for the records
    if E:
        qr, _ = q.positions(R.ray, R.step)
        e_r, a_r = q.alpha_at(qr)
        assert e_r.shape[0] == E and torch.equal(e_r, _cuda(R.exp_d)) and torch.equal(a_r, _cuda(R.alpha))
    again = _Launch(c, q.cfg)
    assert all(torch.equal(x, y) for x, y in zip(q.outputs(), again.outputs()))            # byte for byte
    # the edge the case is in the table for
    n2 = _np(q.n2)
    stopped = _np(q.last).astype(np.float64) < 1e-3
    stop_step = np.array([R.step[R.is_last & (R.ray == r)][0] if stopped[r] else -1 for r in range(N)])
    if c.scene == 'empty' or c.mask_kind == 'false':
        assert not n2.any() and (_np(q.last) == 1).all()
    if c.scene == 'wall':
        assert stopped.all() and (stop_step < 64).all()
    if c.name in ('three162', 'b05_fog'):
        assert (stop_step >= 64).any()
    if c.name == 'carry82':
        assert (R.step == 64).any() and (R.step == 63).any() and cq.shape[0] == E
    if c.name == 'lengths':
        assert tuple(n2) == K.LENGTHS
    print(c.name, 'candidates', cq.shape[0], 'records', E, 'kept', M3, 'stopped rays', int(stopped.sum()))


# ------------------------------------------------------------------------------------------ 2. the model
def _case_models(c, rgbnet_dim=0, seed=0):
    from directvoxgo_amd.dcvgo import DirectContractedVoxGO
    out = []
    for fm in (False, True):
        torch.manual_seed(seed)
        m = DirectContractedVoxGO(c.center - c.radius, c.center + c.radius, num_voxels=c.world ** 3, num_voxels_base=c.world ** 3,
                                  alpha_init=0.5, fast_color_thres=c.thres, bg_len=c.b, contracted_norm=c.norm,
                                  mask_cache_world_size=None if c.mask is None else list(c.mask.shape), rgbnet_dim=rgbnet_dim,
                                  rgbnet_width=64, fused_march=fm)
        out.append(m)
    m0, m1 = out
    assert m0.world == c.world and float(m0.act_shift) == 0.0 and float(m0.voxel_size_ratio) == 1.0
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        m0.density.copy_(torch.from_numpy(c.density)[None, None])
        m0.k0.copy_(torch.randn(m0.k0.shape, generator=g) * 0.5)
    if c.mask is not None:
        m0._set_mask_cache(torch.from_numpy(c.mask))
    m0, m1 = m0.cuda(), m1.cuda()
    m1.load_state_dict(m0.state_dict())
    assert m0.fused_march is False and m1.fused_march is True
    return m0, m1


def _assert_paths_equal(a, b, thres):
    """a: op by op, b: the fused march (see the module docstring for thres == 0)"""
    assert set(a) == set(b) == RESULT_KEYS and a['n_max'] == b['n_max']
    per_sample = ('ray_id', 'step_id', 't', 's', 'weights', 'raw_alpha', 'raw_rgb')
    sel = slice(None)
    if thres == 0:
        key_a, key_b = a['ray_id'] * a['n_max'] + a['step_id'], b['ray_id'] * b['n_max'] + b['step_id']
        sel = torch.isin(key_a, key_b)
        assert int(sel.sum()) == key_b.shape[0] and bool((a['weights'][~sel] == 0).all())
    for k in per_sample:
        assert torch.equal(a[k][sel], b[k]), k
    for k in ('alphainv_last', 'rgb_marched', 'depth'):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_model_paths_agree_on_the_table(c):
    m0, m1 = _case_models(c)
    o, d = _cuda(c.rays_o), _cuda(c.rays_d)
    vd = d / d.norm(dim=-1, keepdim=True)
    rk = dict(near=0.0, far=1e4, stepsize=c.stepsize, bg=0.25, render_depth=True)
    with torch.no_grad():
        a, b = m0(o, d, vd, **rk), m1(o, d, vd, **rk)
    _assert_paths_equal(a, b, c.thres)
    print(c.name, 'op-by-op samples', a['ray_id'].shape[0], 'fused', b['ray_id'].shape[0])


@pytest.fixture(scope='module')
def scene():
    from directvoxgo_amd.scenes import unbounded_scene
    return unbounded_scene(world=64, n_train=4, n_test=0, H=32, W=32)


def _scene_models(sc, **kw):
    from directvoxgo_amd.dcvgo import DirectContractedVoxGO
    args = dict(num_voxels=sc['world'] ** 3, num_voxels_base=sc['world'] ** 3, alpha_init=1e-2, bg_len=sc['bg_len'],
                fast_color_thres=1e-4, rgbnet_dim=12, rgbnet_width=64)
    args.update(kw)
    torch.manual_seed(3)
    m0 = DirectContractedVoxGO([-1, -1, -1], [1, 1, 1], **args)
    m1 = DirectContractedVoxGO([-1, -1, -1], [1, 1, 1], fused_march=True, **args)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        m0.density.copy_(sc['gt'].density.cpu())
        m0.k0.copy_(torch.randn(m0.k0.shape, generator=g) * 0.5)
        for p in m0.rgbnet.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    m0, m1 = m0.cuda(), m1.cuda()
    m1.load_state_dict(m0.state_dict())
    return m0, m1


def test_model_paths_agree_on_the_unbounded_scene(scene):
    sc = scene
    m0, m1 = _scene_models(sc)
    args = (sc['rays_o'], sc['rays_d'], sc['viewdirs'])
    rk = dict(sc['render_kwargs'], render_depth=True)
    with torch.no_grad():
        with _Spy() as s0:
            a = m0(*args, **rk)
        with _Spy() as s1:
            b = m1(*args, **rk)
    assert a['ray_id'].shape[0] > 1000
    _assert_paths_equal(a, b, 1e-4)
    assert 'dvgo_contract_count' in s0.names() and 'dvgo_contract_emit' in s0.names()
    assert s1.names().count('dvgo_march_contract_density') == 1 and 'dvgo_march_gather' in s1.names()
    assert not any(n in s1.names() for n in ('dvgo_contract_count', 'dvgo_contract_emit', 'dvgo_raw2alpha', 'dvgo_alpha2weight'))


# ------------------------------------------------------------------------------------------ 3. the backward kernel
BWD_CASES = [c for c in CASES if c.name in ('three162', 'b05_l2', 'b05_fog', 'lengths')]


@pytest.mark.parametrize('grads', ['random', 'no_last', 'quiet_rays'])
@pytest.mark.parametrize('c', BWD_CASES, ids=[c.name for c in BWD_CASES])
def test_backward_kernel_against_the_tree_reference(c, grads, launches):
    q = launches[c.name][0]
    N, M3, R = q.N, int(q.off3[-1]), q.R
    assert R.ray.shape[0] > 0
    gen = torch.Generator(device='cuda').manual_seed(3)
    gw = torch.randn(M3, device='cuda', generator=gen)
    gl = None if grads != 'random' else torch.randn(N, device='cuda', generator=gen)
    if grads == 'quiet_rays':                      # every other ray without any upstream gradient: the zero rule
        ray_of = torch.repeat_interleave(torch.arange(N, device='cuda'), q.n3.long())
        gw[ray_of % 2 == 0] = 0
    g_raw, q2 = q.backward(gw, gl)
    O = M.density_bwd_reference(R, _np(q.last), M.gw_per_record(R, _np(q.off3), _np(gw)), None if gl is None else _np(gl),
                                c.interval, order='tree')
    assert np.isfinite(O.gd).all() and np.isfinite(O.dgd).all()                            # no record without a bound
    worst = M.check_density_bwd(R, O, _np(g_raw), 'march_contract_density_bwd')
    assert torch.equal(q2, q.positions(R.ray, R.step)[0])
    if grads == 'quiet_rays':
        assert O.zero.any() and (~O.zero).any()
    again = q.backward(gw, gl)
    assert torch.equal(g_raw, again[0]) and torch.equal(q2, again[1])
    print(c.name, grads, 'records', R.ray.shape[0], 'worst err / bound', round(worst, 4))


def test_backward_kernel_ray_lengths(launches):
    assert {1, 63, 64, 65, 129} <= set(int(v) for v in _np(launches['lengths'][0].n2))


# ------------------------------------------------------------------------------------------ 4. model gradients
@pytest.mark.parametrize('rgbnet_dim,direct', [(0, True), (12, True), (12, False)])
def test_fused_forward_and_grads_match_float64(rgbnet_dim, direct):
    """tests/test_gpu_unbounded.py::test_forward_and_grads_match_float64 on the fused path, its model, rays and tolerances
    taken over unchanged.  That model has fast_color_thres == 0: the float64 reference lists the samples behind a ray's stop
    with weight 0, the march does not visit them, so `weights` is compared on the march's samples and the rest of the
    reference's must be exactly 0."""
    import test_gpu_unbounded as TU
    cu = TU.cu
    m = TU._model(rgbnet_dim, direct, fused_march=True)
    assert m.fused_march
    N = 384
    o, d = TU._rays(N, seed=21)
    o = (o * 0.3).astype(np.float32)
    vd = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    rk = dict(near=0.1, far=1e4, stepsize=0.5, bg=0.25, render_depth=True)
    with _Spy() as spy:
        res = m(cu(o), cu(d), cu(vd), global_step=0, **rk)
    assert spy.names().count('dvgo_march_contract_density') == 1 and 'dvgo_contract_emit' not in spy.names()
    rng = np.random.default_rng(2)
    G = rng.normal(size=(N, 3))
    G2 = rng.normal(size=N)
    (res['rgb_marched'] * cu(G.astype(np.float32))).sum().add((res['alphainv_last'] * cu(G2.astype(np.float32))).sum()).backward()

    q, ray_id, step_id, t = m.sample_ray(cu(o), cu(d), 0.5)[:4]
    dens = m.density.detach().cpu().double()[0, 0].requires_grad_(True)
    k0 = m.k0.detach().cpu().double()[0].contiguous().requires_grad_(True)
    head = TU._head64(m)
    interval = float(0.5 * m.voxel_size_ratio)
    ref = U.forward64(q.cpu().numpy(), ray_id.cpu().numpy(), t.cpu().numpy(), N, dens, k0, m.xyz_min.cpu().numpy(),
                      m.xyz_max.cpu().numpy(), float(m.act_shift), interval, 0.25, head, direct, vd, 4)
    (ref['rgb_marched'] * torch.from_numpy(G)).sum().add((ref['alphainv_last'] * torch.from_numpy(G2)).sum()).backward()
    n_max = res['n_max']
    assert n_max == U.t_table(40, 0.5, 0.2)[2]
    sel = torch.isin(ray_id.cpu() * n_max + step_id.cpu(), res['ray_id'].cpu() * n_max + res['step_id'].cpu())
    assert int(sel.sum()) == res['ray_id'].shape[0] > 1000 and bool((ref['weights'].detach()[~sel] == 0).all())
    assert torch.equal(res['ray_id'].cpu(), ray_id.cpu()[sel]) and torch.equal(res['t'].cpu(), t.cpu()[sel])
    assert torch.equal(res['s'].cpu(), (1 - 1 / (1 + t)).cpu()[sel])
    u = 2.0 ** -24
    t_sum = np.bincount(ray_id.cpu().numpy(), weights=t.cpu().double().numpy(), minlength=N)
    n_s = np.bincount(ray_id.cpu().numpy(), minlength=N)
    atol = {'rgb_marched': (8 * u * n_s)[:, None] + 2e-7, 'depth': 8 * u * t_sum + 2e-7, 'weights': 2e-6, 'alphainv_last': 2e-6}
    for k in ('rgb_marched', 'depth', 'weights', 'alphainv_last'):
        got, want = res[k].detach().cpu().double().numpy(), ref[k].detach().numpy()
        if k == 'weights':
            want = want[sel.numpy()]
        assert np.all(np.abs(got - want) <= 1e-5 * np.abs(want) + atol[k]), (k, np.abs(got - want).max())

    def close(got, want, name):
        want = want.numpy()
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-3 * np.abs(want).max(), err_msg=name)
    close(m.density.grad.cpu().double()[0, 0].numpy(), dens.grad, 'density')
    close(m.k0.grad.cpu().double()[0].numpy(), k0.grad, 'k0')
    if head is not None:
        lin = [mod for mod in m.rgbnet.modules() if isinstance(mod, torch.nn.Linear)]
        for i, (l, (W, b)) in enumerate(zip(lin, head)):
            close(l.weight.grad.cpu().double().numpy(), W.grad, f'W{i}')
            close(l.bias.grad.cpu().double().numpy(), b.grad, f'b{i}')


def test_train_step_with_distortion_on_each_path():
    """One TrainStep with weight_distortion > 0 on each path from the same state: the comparison of
    tests/test_gpu_unbounded.py::test_train_step_with_distortion_matches_op_by_op (loss rel 1e-5; parameters rtol 1e-4, atol 1e-5)."""
    import test_gpu_unbounded as TU
    from directvoxgo_amd.train import TrainStep
    cfg = dict(TU.CFG, weight_distortion=0.01)
    rk = dict(near=0, far=1e4, stepsize=0.5, bg=0.5)
    a, b = TU._model(12, True, seed=1, fused_march=True), TU._model(12, True, seed=1)
    before = [p.detach().clone() for p in a.parameters()]
    sa, sb = TrainStep(a, cfg, rk), TrainStep(b, cfg, rk)
    o, d, vd, tgt = TU._batch(seed=20)
    assert sa._plan(o, 1).path == sb._plan(o, 1).path == 'dense' and not sa.can_capture()
    with _Spy() as spy:
        la = sa(o, d, vd, tgt, 1)
    lb = sb(o, d, vd, tgt, 1)
    assert 'dvgo_march_contract_density' in spy.names() and 'dvgo_march_contract_density_bwd' in spy.names()
    assert 'dvgo_distortion_fwd_bwd' in spy.names() and 'dvgo_contract_emit' not in spy.names()
    assert la.item() == pytest.approx(lb.item(), rel=1e-5)
    for (na, pa), (nb, pb) in zip(a.named_parameters(), b.named_parameters()):
        torch.testing.assert_close(pa, pb, rtol=1e-4, atol=1e-5, msg=na)
    assert any(not torch.equal(p, q) for p, q in zip(a.parameters(), before))               # the step moved something


# ------------------------------------------------------------------------------------------ 5. launches, host reads, the rest
def test_one_host_read_and_the_fallback(scene, monkeypatch):
    from directvoxgo_amd import fused as F
    sc = scene
    m0, m1 = _scene_models(sc)
    cfg = m1._march_contract_cfg(0.5, m1.density.device)
    o, d = sc['rays_o'][:1024], sc['rays_d'][:1024]
    reads = []
    for name in ('item', 'tolist', 'cpu', 'numpy', '__int__', '__float__', '__bool__', '__index__'):
        orig = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name, lambda self, *a, _o=orig, _n=name, **k: (reads.append(_n), _o(self, *a, **k))[1])
    with torch.no_grad(), _Spy() as spy:
        out = F.fused_march_contract(m1.density, o, d, cfg)
    monkeypatch.undo()
    assert reads == ['tolist'], reads                                                      # M3 and M2 together
    assert spy.names() == ['dvgo_march_contract_density', 'dvgo_exclusive_scan_i32', 'dvgo_march_gather', 'dvgo_contract_positions']
    w, alpha, last, q, ray_id, step_id, t, off3 = out
    assert q.shape == (w.shape[0], 3) and t.shape == w.shape and off3.shape[0] == 1025 and int(off3[-1]) == w.shape[0] > 0
    # above the scratch budget: None, and the model goes op by op with the same result
    monkeypatch.setattr(F, '_MAX_STRIDE_SCRATCH_BYTES', cfg.n_max * 1024 * 16 - 1)
    assert F.fused_march_contract(m1.density, o, d, cfg) is None
    vd = sc['viewdirs'][:1024]
    with torch.no_grad(), _Spy() as spy:
        b = m1(o, d, vd, **sc['render_kwargs'])
    assert 'dvgo_contract_emit' in spy.names() and 'dvgo_march_contract_density' not in spy.names()
    monkeypatch.undo()
    with torch.no_grad():
        a = m0(o, d, vd, **sc['render_kwargs'])
    assert torch.equal(a['rgb_marched'], b['rgb_marched'])


def test_scale_volume_grid_checkpoint_and_refusals(scene, tmp_path):
    from directvoxgo_amd import fused as F
    from directvoxgo_amd.checkpoint import load_model, save_checkpoint
    from directvoxgo_amd.dcvgo import DirectContractedVoxGO
    sc = scene
    m0, m1 = _scene_models(sc)
    args = (sc['rays_o'][:2048], sc['rays_d'][:2048], sc['viewdirs'][:2048])
    rk = dict(sc['render_kwargs'], render_depth=True)
    for m in (m0, m1):
        m.scale_volume_grid(72 ** 3)
    assert m1.world > 64 and tuple(m1.mask_cache.mask.shape) == (m1.world,) * 3
    with torch.no_grad(), _Spy() as spy:
        b = m1(*args, **rk)
        a = m0(*args, **rk)
    assert spy.names().count('dvgo_march_contract_density') == 1 and b['n_max'] == U.t_table(m1.world, 0.5, sc['bg_len'])[2]
    _assert_paths_equal(a, b, 1e-4)
    assert torch.isfinite(b['rgb_marched']).all() and b['ray_id'].shape[0] > 0
    path = str(tmp_path / 'c.tar')
    save_checkpoint(path, m1, None, 5)
    m2 = load_model(DirectContractedVoxGO, path, fused_march=True).cuda()
    assert m2.fused_march is True and load_model(DirectContractedVoxGO, path).fused_march is False
    with torch.no_grad():
        b2 = m2(*args, **rk)
    assert all(torch.equal(b[k], b2[k]) for k in RESULT_KEYS - {'n_max'})
    with pytest.raises(NotImplementedError, match='DirectContractedVoxGO'):
        m1(args[0].clone().requires_grad_(), args[1], args[2], **rk)
    cfg = m1._march_contract_cfg(0.5, m1.density.device)
    with pytest.raises(NotImplementedError, match='fused_march_contract.*require grad'):
        F.fused_march_contract(m1.density, args[0], args[1].clone().requires_grad_(), cfg)
