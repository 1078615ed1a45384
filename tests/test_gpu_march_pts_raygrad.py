"""GPU: the ray gradient of the fused marches that return positions (csrc/march_raygrad.hip: dvgo_march_ray_bwd_pts,
dvgo_march_vm_ray_bwd), from the kernels to pose.refine_poses(fused=True) for HashVoxGO, VMTriPlaneVoxGO and TensoRFVoxGO.

  dense kernel  called on what a fused_march(positions=True, raygrad=True) forward saved, outputs pre-filled with NaN, every ray
                inside the bound of tests/march_pts_raygrad_oracle.py: the edge-case table (fine129) and the random 20^3 scene with
                96 rays (tests/march_pts_raygrad_cases.py), fixed-stride and exact layout, grad_pts given and NULL, grad_last given
                and NULL; with grad_pts NULL the bits of dvgo_march_ray_bwd(C = 0); a second launch repeats the bits; N = 5, N = 0
  VM kernel     on the records of dvgo_march_vm_density: the tables fine129 / coarse129, padded R (float4) and unpadded, and the
                random scene with six non-zero tensors, R = 4 and R = 5, channels-last and contiguous with the same bits; N = 5,
                N = 0; repeatable
  fused.py      raygrad=True: the outputs' bits, what the scatters read and give, the defaults' refusals before any launch
  models        raygrad='fused': the fused forward's bits in every key, rays_o.grad / rays_d.grad against the float64 restatements of
                tests/test_gpu_hash_raygrad.py / tests/test_gpu_vm_raygrad.py by their rule, the launch log
  refine_poses  fused=True recovers those files' captures with the model frozen; poses and model step together through a TrainStep
The worst err / bound per kernel case is printed (pytest -s): information, never a threshold.
"""
import math

import numpy as np
import pytest
import torch

import hash_render_oracle as RO
import march_cases as C
import march_oracle as M
import march_pts_raygrad_cases as PC
import march_pts_raygrad_oracle as PO
import march_vm_cases as V
import test_gpu_hash_raygrad as TH
import test_gpu_vm_raygrad as TV
import vm_density_oracle as DO
from test_gpu_march_raygrad import _Calls, _launch as _launch_k0, _records, _stride_layout, _t_min
from test_gpu_march_vm import _check_six, _Launch, _lay, _scene_cfg
from test_gpu_raygrad import _dict_bits_equal, cu, host, same_bits

pytestmark = pytest.mark.gpu
KEYS = V.KEYS


# ------------------------------------------------------------------------------------------ the dense kernel
def _dense_scene(which):
    from directvoxgo_amd import fused as F
    sc = C.fine_scene() if which == 'fine129' else PC.rand20_scene()
    density = cu(sc.density)[None, None].contiguous()
    cfg = F.MarchConfig(cu(sc.xyz_min), cu(sc.xyz_max), sc.stepdist, sc.act_shift, sc.interval, sc.thres, sc.near, sc.far,
                        mask=cu(sc.mask), xyz2ijk_scale=cu(sc.mask_scale), xyz2ijk_shift=cu(sc.mask_shift))
    o, d = (cu(a) for a in sc.arrays())
    return sc, density, cfg, o, d


def _no_k0(density):
    return torch.zeros((1, 0, *density.shape[2:]), device='cuda')


def _forward(density, o, d, cfg):
    """fused_march(positions=True, raygrad=True) with rays that require grad -> (what it saved, rec_stride, positions)"""
    from directvoxgo_amd import fused as F
    ro, rd = o.clone().requires_grad_(), d.clone().requires_grad_()
    w, alpha, last, pts, ray_id, step_id, off3 = F.fused_march(density, _no_k0(density), ro, rd, cfg, positions=True, raygrad=True)
    fn = w.grad_fn
    assert fn.pts_grad and not fn.ray_grad and len(fn.saved_tensors) == 12 and pts.requires_grad and pts.shape == (w.shape[0], 3)
    assert same_bits(fn.saved_tensors[10], o) and same_bits(fn.saved_tensors[11], d)
    return fn.saved_tensors, fn.geom[8], pts


def _launch_pts(L, saved, stride, cfg, o, d, density, gw, gl, gpts, N):
    rec2, n2, n_steps, cum, off3, start, dirs, last = saved[:8]
    X, Y, Z = density.shape[2:]
    go = torch.full((max(N, 1), 3), float('nan'), device='cuda')
    gd = torch.full((max(N, 1), 3), float('nan'), device='cuda')
    L.call('dvgo_march_ray_bwd_pts', rec2, n2, n_steps, cum if stride == 0 else None, stride, off3, N, start, dirs, cfg.stepdist,
           cfg.xyz_min_h, cfg.xyz_max_h, last, cfg.interval, o, d, cfg.near, cfg.far, density, X, Y, Z, gw, gl, gpts, go, gd,
           L.stream_of(go))
    torch.cuda.synchronize()
    return host(go), host(gd)


def _box(cfg):
    return np.array(list(cfg.xyz_min_h), np.float32), np.array(list(cfg.xyz_max_h), np.float32)


@pytest.mark.parametrize('layout', ['stride', 'exact'])
@pytest.mark.parametrize('which', ['fine129', 'rand20'])
def test_dense_kernel_inside_the_oracle_bound(which, layout):
    from directvoxgo_amd import _lib as L
    sc, density, cfg, o, d = _dense_scene(which)
    N = o.shape[0]
    with _stride_layout(layout):
        saved, stride, _ = _forward(density, o, d, cfg)
    assert (stride == 0) == (layout == 'exact')
    Rc, n_steps = _records(saved, stride)
    off3, last = host(saved[4])[:N + 1], host(saved[7])
    M3 = int(off3[-1])
    n3 = np.bincount(Rc.ray, Rc.flag, N).astype(np.int64)
    if which == 'fine129':                                      # the chunk and stop cases are there, on the device's records
        q = C.Result(Rc, n3, last, n_steps, host(saved[5]))
        for name, target, pred in sc.rows:
            assert pred(q), f'row {name} ({target}) does not hit its edge on the device'
        assert {0, 1, 63, 64, 65, 256} <= set(Rc.n.tolist())
        assert {63, 64, 127, 192} <= {q.stopped_at(r) for r in range(N)}          # lane 63 of a chunk, lane 0 of the next
    else:
        assert N == 96 and Rc.ray.shape[0] >= M3 > 300
    assert np.any((n3 > 0) & (n3 < Rc.n))                       # flagged and unflagged records in one ray
    t_min = _t_min(o, d, cfg)
    gw_np, gl_np, gp_np = PC.upstream(N, M3, 41)
    gw, gl, gp = cu(gw_np), cu(gl_np), cu(gp_np)
    gwr = M.gw_per_record(Rc, off3, gw_np)
    mn, mx = _box(cfg)
    for with_last, with_pts in ((True, True), (False, True), (True, False), (False, False)):
        go, gd = _launch_pts(L, saved, stride, cfg, o, d, density, gw, gl if with_last else None, gp if with_pts else None, N)
        G = PO.reference_dense(Rc, last, gwr, gl_np if with_last else None, cfg.interval, host(saved[5]), host(saved[6]), cfg.stepdist,
                               mn, mx, host(density)[0, 0], PO.pts_rows(Rc, off3, gp_np) if with_pts else None, t_min, host(d))
        assert G.finite.all() and float(np.abs(G.A).max()) > 1e-3 and float(np.abs(G.B).max()) > 1e-3
        what = f'{which} {layout} grad_last={with_last} grad_pts={with_pts}'
        print(f'\nworst err / bound  {what}: {PO.check(G, go, gd, (), what=what):.4f}', end='')
        again = _launch_pts(L, saved, stride, cfg, o, d, density, gw, gl if with_last else None, gp if with_pts else None, N)
        assert same_bits(go, again[0]) and same_bits(gd, again[1])                # repeatable
        if not with_pts:                                        # the bits of dvgo_march_ray_bwd without a feature term
            k0 = _launch_k0(L, saved, stride, cfg, o, d, density, _no_k0(density), gw, gl if with_last else None, None, N)
            assert same_bits(go, k0[0]) and same_bits(gd, k0[1])


def test_dense_kernel_partly_filled_workgroup_and_no_rays():
    """N = 5: two workgroups of four wavefronts, the second with one ray; N = 0: nothing is launched or written"""
    from directvoxgo_amd import _lib as L
    sc, density, cfg, o, d = _dense_scene('fine129')
    o, d = o[:5].contiguous(), d[:5].contiguous()
    saved, stride, _ = _forward(density, o, d, cfg)
    Rc, _ = _records(saved, stride)
    assert Rc.n.tolist()[0] == 0 and Rc.n.shape[0] == 5 and Rc.ray.shape[0] > 60
    off3, last = host(saved[4])[:6], host(saved[7])
    gw_np, gl_np, gp_np = PC.upstream(5, int(off3[-1]), 43)
    gw, gl, gp = cu(gw_np), cu(gl_np), cu(gp_np)
    go, gd = _launch_pts(L, saved, stride, cfg, o, d, density, gw, gl, gp, 5)
    mn, mx = _box(cfg)
    G = PO.reference_dense(Rc, last, M.gw_per_record(Rc, off3, gw_np), gl_np, cfg.interval, host(saved[5]), host(saved[6]), cfg.stepdist,
                           mn, mx, host(density)[0, 0], PO.pts_rows(Rc, off3, gp_np), _t_min(o, d, cfg), host(d))
    print(f'\nworst err / bound  N=5: {PO.check(G, go, gd, (), what="N=5"):.4f}', end='')
    go0, gd0 = _launch_pts(L, saved, stride, cfg, o, d, density, gw, gl, gp, 0)
    assert np.all(np.isnan(go0)) and np.all(np.isnan(gd0))


# ------------------------------------------------------------------------------------------ the VM kernel
def _vm_launch(L, q, planes, lines, o, d, gw, gl, gpts, N=None):
    from directvoxgo_amd.ops import _line_geom, _plane_pack
    N = q.N if N is None else N
    g = _plane_pack([planes[k] for k in KEYS])
    for k in KEYS:
        g += [lines[k], *_line_geom(lines[k], k + '_line')]
    cfg = q.cfg
    go = torch.full((max(N, 1), 3), float('nan'), device='cuda')
    gd = torch.full((max(N, 1), 3), float('nan'), device='cuda')
    L.call('dvgo_march_vm_ray_bwd', q.rec2, q.n2, q.stride, q.off3, N, q.start, q.dirs, cfg.stepdist, cfg.xyz_min_h, cfg.xyz_max_h,
           q.last, cfg.interval, o, d, cfg.near, cfg.far, *g, planes['xy'].shape[1], gw, gl, gpts, go, gd, L.stream_of(go))
    torch.cuda.synchronize()
    return host(go), host(gd)


def _vm_check(L, name, sc, planes_np, lines_np, layouts, N=None):
    """One scene: the forward's records, then every (grad_last, grad_pts) combination in every layout of `layouts`."""
    o, d = (cu(a) for a in sc.arrays())
    if N is not None:
        o, d = o[:N].contiguous(), d[:N].contiguous()
    cfg = _scene_cfg(sc)
    first = None
    for layout in layouts:
        dp, dl = {k: _lay(planes_np[k], layout) for k in KEYS}, {k: _lay(lines_np[k], layout) for k in KEYS}
        assert (dp['xy'].stride(1) == 1) == (layout == 'cl') or dp['xy'].shape[1] == 1
        q = _Launch(cfg, dp, dl, o, d)
        Rc, off3 = q.R, host(q.off3)
        M3 = int(off3[-1])
        gw_np, gl_np, gp_np = PC.upstream(q.N, M3, 47)
        gw, gl, gp = cu(gw_np), cu(gl_np), cu(gp_np)
        t_min = _t_min(o, d, cfg)
        mn, mx = _box(cfg)
        got = {}
        for with_last, with_pts in ((True, True), (False, False)):
            go, gd = _vm_launch(L, q, dp, dl, o, d, gw, gl if with_last else None, gp if with_pts else None)
            if first is None or layout == layouts[0]:
                G = PO.reference_vm(Rc, host(q.last), M.gw_per_record(Rc, off3, gw_np), gl_np if with_last else None, cfg.interval,
                                    host(q.start), host(q.dirs), cfg.stepdist, mn, mx, planes_np, lines_np,
                                    PO.pts_rows(Rc, off3, gp_np) if with_pts else None, t_min, host(d))
                assert G.finite.all() and float(np.abs(G.A).max()) > 1e-3 and float(np.abs(G.B).max()) > 1e-3
                what = f'{name} {layout} grad_last={with_last} grad_pts={with_pts}'
                print(f'\nworst err / bound  {what}: {PO.check(G, go, gd, (), what=what):.4f}', end='')
            again = _vm_launch(L, q, dp, dl, o, d, gw, gl if with_last else None, gp if with_pts else None)
            assert same_bits(go, again[0]) and same_bits(gd, again[1])            # repeatable
            got[with_last, with_pts] = (go, gd)
        if first is None:
            first = got
        else:                                                   # the layout changes no bit
            for key in got:
                assert same_bits(first[key][0], got[key][0]) and same_bits(first[key][1], got[key][1]), (name, layout, key)
    return q, Rc


@pytest.mark.parametrize('pad', [True, False], ids=['padded', 'unpadded'])
@pytest.mark.parametrize('which', ['fine129', 'coarse129'])
def test_vm_kernel_on_the_edge_case_tables(which, pad):
    from directvoxgo_amd import _lib as L
    sc = C.fine_scene() if which == 'fine129' else C.coarse_scene()
    planes, lines = V.vm_tensors(sc, pad)
    R = planes['xy'].shape[1]
    assert R == V.TABLE[sc.name][0 if pad else 1] and (R % 4 == 0) == pad
    q, Rc = _vm_check(L, f'{which} R={R}', sc, planes, lines, ['cl', 'cf'])        # padded + 'cl': the float4 path
    assert Rc.ray.shape[0] == V.TABLE[sc.name][3]
    if which == 'fine129':
        assert {0, 1, 63, 64, 65, 256} <= set(Rc.n.tolist())
        res = q.result
        assert {63, 64, 127, 192} <= {res.stopped_at(r) for r in range(q.N)}
        n3 = host(q.n3).astype(np.int64)
        assert np.any((n3 > 0) & (n3 < Rc.n))


@pytest.mark.parametrize('R', [4, 5])
def test_vm_kernel_on_six_random_tensors(R):
    from directvoxgo_amd import _lib as L
    sc, planes, lines = PC.vm20_scene(R)
    assert all(float(np.abs(t).min()) > 0 for t in list(planes.values()) + list(lines.values()))
    q, Rc = _vm_check(L, sc.name, sc, planes, lines, ['cl', 'cf'])
    assert q.N == 96 and Rc.ray.shape[0] > 1000 and int(q.off3[-1]) > 300


def test_vm_kernel_partly_filled_workgroup_and_no_rays():
    from directvoxgo_amd import _lib as L
    sc, planes, lines = PC.vm20_scene(4)
    q, Rc = _vm_check(L, 'vm20 N=5', sc, planes, lines, ['cl'], N=5)
    assert q.N == 5 and Rc.ray.shape[0] > 20
    dp, dl = {k: _lay(planes[k], 'cl') for k in KEYS}, {k: _lay(lines[k], 'cl') for k in KEYS}
    o, d = (cu(a)[:5].contiguous() for a in sc.arrays())
    M3 = int(q.off3[-1])
    gw, gl, gp = (cu(a) for a in PC.upstream(5, M3, 47))
    go0, gd0 = _vm_launch(L, q, dp, dl, o, d, gw, gl, gp, N=0)
    assert np.all(np.isnan(go0)) and np.all(np.isnan(gd0))


# ------------------------------------------------------------------------------------------ fused.py
def test_fused_march_positions_raygrad_keeps_bits_and_what_the_scatter_reads():
    """raygrad=True with rays that require grad: every output has the bits of the default call on detached rays; the density
    scatter (float atomics: not repeatable) reads the same bits and stays inside march_oracle's bound (MarchSpy holds every
    dvgo_march_density_bwd to it); dvgo_march_ray_bwd_pts is the first launch of the backward and its result repeats."""
    from directvoxgo_amd import fused as F
    sc, density, cfg, o, d = _dense_scene('rand20')
    none = _no_k0(density)
    plain = F.fused_march(density, none, o, d, cfg, positions=True)
    runs = []
    for need in (False, True, True):
        dens = density.clone().requires_grad_()
        ro, rd = o.clone().requires_grad_(need), d.clone().requires_grad_(need)
        out = F.fused_march(dens, none, ro, rd, cfg, positions=True, raygrad=True)
        for a, b in zip(plain, out):
            assert same_bits(a, b.detach())
        assert out[3].requires_grad == need
        gen = torch.Generator(device='cuda').manual_seed(5)
        gw, gl = torch.randn(out[0].shape, device='cuda', generator=gen), torch.randn(out[2].shape, device='cuda', generator=gen)
        gp = torch.randn(out[3].shape, device='cuda', generator=gen)
        seen = {}
        with M.MarchSpy(check=True) as spy:
            call = spy._L.call

            def tap(name, *args):
                if name == 'dvgo_march_density_bwd':
                    ix = M.B.param_index(name)
                    seen['gw'], seen['gl'] = (host(args[ix[k]]).copy() for k in ('grad_weights', 'grad_last'))
                return call(name, *args)
            spy._L.call = tap
            torch.autograd.backward([out[0], out[2]] + ([out[3]] if need else []), [gw, gl] + ([gp] if need else []))
            torch.cuda.synchronize()
        names = [n for n in spy.calls if n.startswith('dvgo_march')]
        assert names == (['dvgo_march_ray_bwd_pts'] if need else []) + ['dvgo_march_density_bwd'], spy.calls
        runs.append(dict(gd=dens.grad.clone(), go=ro.grad, gr=rd.grad, **seen))
    base, first, second = runs
    assert base['go'] is None and float(base['gd'].abs().sum()) > 0
    for other in (first, second):
        assert same_bits(base['gw'], other['gw']) and same_bits(base['gl'], other['gl'])         # what the scatter reads
        assert float(other['gd'].abs().sum()) > 0                # (each pass's density.grad was held to the oracle's bound: MarchSpy)
    assert same_bits(first['go'], second['go']) and same_bits(first['gr'], second['gr'])
    assert float(first['go'].abs().sum()) > 0 and bool(torch.isfinite(first['gr']).all())


def test_fused_march_vm_raygrad_keeps_bits_and_runs_with_a_frozen_model():
    from directvoxgo_amd import fused as F
    sc, planes, lines = PC.vm20_scene(4)
    cfg = _scene_cfg(sc)
    o, d = (cu(a) for a in sc.arrays())
    mn, mx = _box(cfg)

    def tensors(grad):
        return ({k: _lay(planes[k], 'cl').requires_grad_(grad) for k in KEYS}, {k: _lay(lines[k], 'cl').requires_grad_(grad) for k in KEYS})
    dp, dl = tensors(False)
    plain = F.fused_march_vm(dp, dl, o, d, cfg)
    assert plain is not None and plain[0].numel() > 300
    gen = torch.Generator(device='cuda').manual_seed(5)
    gw, gl = torch.randn(plain[0].shape, device='cuda', generator=gen), torch.randn(plain[2].shape, device='cuda', generator=gen)
    gp = torch.randn(plain[3].shape, device='cuda', generator=gen)
    runs = []
    for model, need in ((True, False), (True, True), (False, True), (True, True)):
        dp, dl = tensors(model)
        ro, rd = o.clone().requires_grad_(need), d.clone().requires_grad_(need)
        out = F.fused_march_vm(dp, dl, ro, rd, cfg, raygrad=True)
        for a, b in zip(plain, out):
            assert same_bits(a, b.detach())
        assert out[3].requires_grad == need
        with _Calls() as calls:
            args = {}
            call = calls._L.call

            def tap(name, *a):
                if name == 'dvgo_vm_density_bwd':
                    args['g_raw'], args['xyz2'] = host(a[0]).copy(), host(a[-7]).copy()
                return call(name, *a)
            calls._L.call = tap
            torch.autograd.backward([out[0], out[2]] + ([out[3]] if need else []), [gw, gl] + ([gp] if need else []))
            torch.cuda.synchronize()
        want = (['dvgo_march_vm_ray_bwd'] if need else []) + (['dvgo_march_vm_density_bwd', 'dvgo_vm_density_bwd'] if model else [])
        assert calls.names == want, calls.names
        if model:                                               # the six gradients: tests/test_gpu_march_vm.py's bound
            live = args['g_raw'] != 0
            ref = DO.backward(planes, lines, args['xyz2'][live], mn, mx, args['g_raw'][live])
            _check_six({**{k: dp[k].grad for k in KEYS}, **{k + '_line': dl[k].grad for k in KEYS}}, ref, ('vm20', need))
        runs.append(dict(go=ro.grad, gr=rd.grad, **args))
    base, with_model, frozen, again = runs
    assert base['go'] is None and frozen['go'] is not None and 'g_raw' not in frozen
    for other in (with_model, again):                           # what the scatter reads keeps its bits
        assert same_bits(base['g_raw'], other['g_raw']) and same_bits(base['xyz2'], other['xyz2'])
    for other in (frozen, again):                               # the ray gradients: frozen or not, once or twice
        assert same_bits(with_model['go'], other['go']) and same_bits(with_model['gr'], other['gr'])
    assert float(frozen['go'].abs().sum()) > 0 and bool(torch.isfinite(frozen['gr']).all())


def test_default_calls_still_refuse_such_rays_before_any_launch():
    from directvoxgo_amd import fused as F
    sc, density, cfg, o, d = _dense_scene('rand20')
    with _Calls() as calls, pytest.raises(NotImplementedError, match='positional'):
        F.fused_march(density, _no_k0(density), o, d.clone().requires_grad_(), cfg, positions=True)
    sc, planes, lines = PC.vm20_scene(4)
    dp, dl = {k: cu(planes[k]) for k in KEYS}, {k: cu(lines[k]) for k in KEYS}
    with _Calls() as calls2, pytest.raises(NotImplementedError, match='fused_march_vm.*require grad'):
        F.fused_march_vm(dp, dl, o.clone().requires_grad_(), d, _scene_cfg(sc))
    assert calls.names == [] and calls2.names == []


# ------------------------------------------------------------------------------------------ the models
def _model(which, seed, **kw):
    if which == 'hash':
        return RO.make_model(32, seed, **kw).cuda()
    return TV.make_model(which, 32, seed=seed, **({'fused_march': True} if which == 'tensorf' else {}), **kw).cuda()


def _scene_rays():
    from directvoxgo_amd import scenes
    sc = scenes.synthetic_scene(world=32, n_rays=256)
    return sc['rays_o'].cuda(), sc['rays_d'].cuda(), sc['viewdirs'].cuda()


ENTRY = {'hash': 'dvgo_march_ray_bwd_pts', 'vm': 'dvgo_march_ray_bwd_pts', 'tensorf': 'dvgo_march_vm_ray_bwd'}


@pytest.mark.parametrize('which', ['hash', 'vm', 'tensorf'])
def test_model_keeps_the_fused_forward_and_its_ray_gradients_match_the_float64_restatement(which):
    """The rule of tests/test_gpu_hash_raygrad.py / tests/test_gpu_vm_raygrad.py, with their restatements and device records:
    the device's error at most 4 x the float32 restatement's own, and the share of the gradient through the features / VM
    tensors above 100 x that tolerance on at least half of the rays that reach a kept sample."""
    T = TH if which == 'hash' else TV
    RK = T.RK
    o, d, v = _scene_rays()
    m = _model(which, 3, raygrad='fused')
    assert m.fused and m.raygrad and m.fused_raygrad
    with torch.no_grad():
        plain = m(o, d, v, **RK)                                 # the fused forward
    ro, rd = o.clone().requires_grad_(), d.clone().requires_grad_()
    with _Calls() as calls:
        res = m(ro, rd, v, **RK)
        res['rgb_marched'].square().sum().backward()
    _dict_bits_equal(plain, {k: t.detach() for k, t in res.items()})
    assert calls.names.count(ENTRY[which]) == 1
    assert 'dvgo_grid_sample_bwd_xyz' not in calls.names and 'dvgo_vm_density_bwd_xyz' not in calls.names
    assert ('dvgo_march_vm_density' if which == 'tensorf' else 'dvgo_march_density') in calls.names
    assert ro.grad is not None and rd.grad is not None
    rec = T._device_record(m, o, d)
    assert same_bits(rec['ray_id0'][rec['m1']][rec['m2']], res['ray_id'])         # the record is this forward's
    o64, d64, marched64 = T._ray_grads(m, o, d, v, rec, torch.float64)
    o32, d32, _ = T._ray_grads(m, o, d, v, rec, torch.float32)
    on, dn, _ = T._ray_grads(m, o, d, v, rec, torch.float64, False)               # without the features' / VM tensors' positions
    assert float((marched64 - res['rgb_marched'].detach().cpu().double()).abs().max()) < 1e-4
    hit = torch.zeros(len(o), dtype=torch.bool)
    hit[res['ray_id'].cpu()] = True
    assert int(hit.sum()) >= 64
    for what, g64, g32, gn, dev in (('rays_o.grad', o64, o32, on, ro.grad), ('rays_d.grad', d64, d32, dn, rd.grad)):
        e32 = float((g32 - g64).abs().max())
        err = float((dev.detach().cpu().double() - g64).abs().max())
        share = (g64 - gn).abs().amax(-1)
        frac = float((share[hit] > 100 * 4 * e32).float().mean())
        print(f'\nfused {which} {what}: max |g64| {float(g64.abs().max()):.4g}  e32 {e32:.4g}  device error {err:.4g}  (allowed '
              f'{4 * e32:.4g})  share above 100 x allowed on {frac:.2f} of the {int(hit.sum())} rays with samples', end='')
        assert float(g64.abs().max()) > 1e-3 and e32 > 0
        assert err <= 4 * e32, (what, err, e32)
        assert frac >= 0.5, (what, frac)


# ------------------------------------------------------------------------------------------ refine_poses(fused=True)
def _capture(which, m):
    if which == 'hash':
        from directvoxgo_amd.pose import CameraRefiner
        true, noisy, HW, Ks = RO.capture(**TH.CAPTURE)
        n, hw = len(true), int(HW[0, 0])
        exact = CameraRefiner(true, HW, Ks).cuda()
        view = torch.arange(n, device='cuda').repeat_interleave(hw * hw)
        p = torch.arange(hw * hw, device='cuda').repeat(n)
        with torch.no_grad():
            o, d, v = exact.rays(view, p % hw, p // hw)
            images = m(o, d, v, **TH.RK_POSE)['rgb_marched'].reshape(n, hw, hw, 3)
        assert float(images.std()) > 0.05
        return true, noisy, HW, Ks, images
    return TV._capture(m)


def _train_cfg(which):
    from directvoxgo_amd.hashgrid import HASH_FINE_TRAIN
    from directvoxgo_amd.tensorf import TENSORF_FINE_TRAIN
    return dict(HASH_FINE_TRAIN if which == 'hash' else TENSORF_FINE_TRAIN)


@pytest.mark.parametrize('which', ['hash', 'vm', 'tensorf'])
def test_refine_poses_fused_recovers_a_perturbed_capture(which):
    """The captures, iteration count, learning rate and thresholds of the op-by-op recovery tests of
    tests/test_gpu_hash_raygrad.py / tests/test_gpu_vm_raygrad.py, on the fused march with the model frozen."""
    from directvoxgo_amd.pose import CameraRefiner, refine_poses
    T = TH if which == 'hash' else TV
    m = _model(which, T.MODEL_SEED, raygrad='fused')
    for p in m.parameters():
        p.requires_grad_(False)
    true, noisy, HW, Ks, images = _capture(which, m)
    ref = CameraRefiner(noisy, HW, Ks).cuda()
    rot0, tr0 = RO.pose_errors(ref.poses(), true)
    cfg = dict(_train_cfg(which), weight_entropy_last=0.0, weight_rgbper=0.0)
    with _Calls() as calls:
        losses = refine_poses(m, ref, images, cfg, T.RK_POSE, n_iters=200, n_rand=None, lrate_pose=T.LRATE_POSE, fused=True)
    rot1, tr1 = RO.pose_errors(ref.poses(), true)
    print(f'\nrefine_poses(fused=True) {which}: loss {losses[0]:.3e} -> {losses[-1]:.3e}; rotation error (deg) '
          f'{np.degrees(rot0.numpy()).round(3).tolist()} -> {np.degrees(rot1.numpy()).round(3).tolist()}; translation error '
          f'{tr0.numpy().round(4).tolist()} -> {tr1.numpy().round(4).tolist()}', end='')
    assert calls.names.count(ENTRY[which]) == 200
    assert 'dvgo_grid_sample_bwd_xyz' not in calls.names and 'dvgo_vm_density_bwd_xyz' not in calls.names
    assert m.__dict__.get('fused_raygrad') is True               # as found
    assert len(losses) == 200 and all(math.isfinite(x) for x in losses)
    assert losses[-1] < losses[0]
    assert bool((rot1 < rot0).all()) and bool((tr1 < tr0).all())
    assert all(q.grad is None for q in m.parameters())           # a frozen model is left alone


@pytest.mark.parametrize('which', ['hash', 'vm', 'tensorf'])
def test_refine_poses_fused_steps_poses_and_model_through_a_train_step(which, monkeypatch):
    from directvoxgo_amd import train
    from directvoxgo_amd.pose import CameraRefiner, refine_poses
    T = TH if which == 'hash' else TV
    steps = []

    class Recorded(train.TrainStep):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            steps.append(self)
    monkeypatch.setattr(train, 'TrainStep', Recorded)
    m = _model(which, T.MODEL_SEED, raygrad='fused')
    true, noisy, HW, Ks, images = _capture(which, m)
    ref = CameraRefiner(noisy, HW, Ks).cuda()
    before = [p.detach().clone() for p in m.parameters()]
    with _Calls() as calls:
        losses = refine_poses(m, ref, images, _train_cfg(which), T.RK_POSE, n_iters=20, n_rand=1024, lrate_pose=T.LRATE_POSE,
                              train_model=True, seed=1, fused=True)
    assert len(steps) == 1 and calls.names.count(ENTRY[which]) == 20
    assert len(losses) == 20 and all(math.isfinite(x) for x in losses) and losses[-1] < losses[0]
    assert sum(not torch.equal(a, b.detach()) for a, b in zip(before, m.parameters())) >= len(before) // 2
    g = ref.delta.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().sum()) > 0 and float(ref.delta.detach().abs().sum()) > 0
    assert m.__dict__.get('fused_raygrad') is True
