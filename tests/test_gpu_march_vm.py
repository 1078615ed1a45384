"""GPU: the fused march over the decomposed density (csrc/march_vm.hip), `fused.fused_march_vm` and
`TensoRFVoxGO(fused_march=True)`.

  1. the edge-case table (tests/march_vm_cases.py: three scenes, padded and unpadded R, channel-first and channels-last)
     through the entry point itself: tests/march_oracle.py's exact statements on the records (T recurrence, stop rule, flags,
     n3, alphainv_last), `check_gather` behind dvgo_march_gather, every row's predicate on the device's records, n2 / n3 /
     steps / flags equal to the host restatement's, two launches byte for byte the same;
  2. the bits of the density: exp_d and alpha of every record equal dvgo_raw2alpha of dvgo_vm_density_fwd at the record's
     position, on the table and on a random scene with R = 3 and 4;
  3. the backward kernel against `march_oracle.density_bwd_reference(order='tree')`, every record, the derived bound and the
     zero rule; positions bit-equal to `march_positions`; rays of 1, 63, 64, 65, 129 and more than 512 records;
  4. the six gradients of the autograd function against `vm_density_oracle.backward` fed the kernel's own g_raw, inside
     tests/test_gpu_vm_density.py's bound (n + 12) U A per texel and node, exact zero where nothing contributes;
  5. the model: both paths from one state dict give equal tensors; what the fused forward launches; gradients; overrides;
     TrainStep, scale_volume_grid, the refusals.
Every bound is derived where it is stated (march_oracle.py, test_gpu_vm_density.py); none was fitted to this kernel.
"""
import contextlib

import numpy as np
import pytest
import torch

import march_cases as C
import march_oracle as M
import march_vm_cases as V
import vm_density_oracle as DO
import vm_oracle as VO

pytestmark = pytest.mark.gpu

SCENES = V.scenes()
KEYS = VO.KEYS
AMP, SIGMA, OFFSET = 20.0, 0.6, -9.0


def _cuda(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda', dtype=dtype)


def _lay(p, layout):
    t = _cuda(p)
    return t.contiguous(memory_format=torch.channels_last) if layout == 'cl' else t


def _np(t):
    return t.detach().cpu().numpy()


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


def _scene_cfg(sc):
    from directvoxgo_amd import fused as F
    return F.MarchConfig(_cuda(sc.xyz_min), _cuda(sc.xyz_max), sc.stepdist, sc.act_shift, sc.interval, sc.thres, sc.near, sc.far,
                         mask=_cuda(sc.mask, torch.bool), xyz2ijk_scale=_cuda(sc.mask_scale), xyz2ijk_shift=_cuda(sc.mask_shift))


class _Launch:
    """One dvgo_march_vm_density through `_lib.call` -> the device's outputs, the `Records` and the `Result` of them."""

    def __init__(self, cfg, planes, lines, o, d):
        from directvoxgo_amd import _lib as L
        from directvoxgo_amd import fused as F
        from directvoxgo_amd.ops import _line_geom, _plane_pack
        N = o.shape[0]
        self.N, self.cfg, self.stride = N, cfg, F._rec_stride(cfg, N)
        assert self.stride > 0
        g = _plane_pack([planes[k] for k in KEYS])
        for k in KEYS:
            g += [lines[k], *_line_geom(lines[k], k + '_line')]
        R = planes['xy'].shape[1]
        dev = o.device
        self.n_steps = torch.zeros(N, dtype=torch.int64, device=dev)
        self.start, self.dirs = torch.zeros((N, 3), device=dev), torch.zeros((N, 3), device=dev)
        self.n2, self.n3 = torch.zeros(N, dtype=torch.int32, device=dev), torch.zeros(N, dtype=torch.int32, device=dev)
        self.last = torch.zeros(N, device=dev)
        self.rec2 = torch.zeros((self.stride * N, 4), device=dev)
        m = cfg.mask
        L.call('dvgo_march_vm_density', self.start, self.dirs, self.n_steps, self.stride, N, cfg.xyz_min_h, cfg.xyz_max_h,
               cfg.stepdist, m, m.shape[0], m.shape[1], m.shape[2], cfg.scale_h, cfg.shift_h, *g, R, cfg.act_shift, cfg.interval,
               cfg.thres, self.rec2, self.n2, self.n3, self.last, o, d, cfg.near, cfg.far, L.stream_of(o))
        torch.cuda.synchronize()
        self.R = M.Records(_np(self.rec2), _np(self.n2), np.arange(N, dtype=np.int64) * self.stride)
        self.result = C.Result(self.R, _np(self.n3), _np(self.last), _np(self.n_steps), _np(self.start))
        self.off3 = torch.zeros(N + 1, dtype=torch.int64, device=dev)
        self.off3[1:] = torch.cumsum(self.n3, 0)
        self.off2 = torch.zeros(N + 1, dtype=torch.int64, device=dev)
        self.off2[1:] = torch.cumsum(self.n2, 0)

    def outputs(self):
        return (self.rec2, self.n2, self.n3, self.last, self.n_steps, self.start, self.dirs)

    def record_positions(self):
        """march_positions of every record, in the order of `Records` (ray-major): [M2, 3]"""
        from directvoxgo_amd.shade import march_positions
        return march_positions(self.start, self.dirs, _cuda(self.R.ray, torch.int64), _cuda(self.R.step, torch.int64),
                               self.cfg.stepdist)

    def gather(self):
        from directvoxgo_amd import _lib as L
        M3 = int(self.off3[-1])
        dev = self.rec2.device
        ray_id, step_id = torch.zeros(M3, dtype=torch.int64, device=dev), torch.zeros(M3, dtype=torch.int64, device=dev)
        w, a = torch.zeros(M3, device=dev), torch.zeros(M3, device=dev)
        cfg = self.cfg
        L.call('dvgo_march_gather', self.rec2, self.n2, self.n_steps, None, self.stride, self.off3, self.N, M3, self.start,
               self.dirs, cfg.stepdist, cfg.xyz_min_h, cfg.xyz_max_h, None, 0, 1, 1, 1, 1, 1, 1, 1, ray_id, step_id, w, a, None,
               L.stream_of(w))
        torch.cuda.synchronize()
        return ray_id, step_id, w, a

    def backward(self, gw, gl):
        """dvgo_march_vm_density_bwd -> (g_raw [M2], xyz2 [M2, 3])"""
        from directvoxgo_amd import _lib as L
        M2 = int(self.off2[-1])
        dev = self.rec2.device
        g_raw, xyz2 = torch.full((M2,), float('nan'), device=dev), torch.full((M2, 3), float('nan'), device=dev)
        cfg = self.cfg
        L.call('dvgo_march_vm_density_bwd', self.rec2, self.n2, self.n_steps, self.stride, self.off3, self.off2, self.N, self.start,
               self.dirs, cfg.stepdist, self.last, cfg.interval, gw, gl, g_raw, xyz2, L.stream_of(g_raw))
        torch.cuda.synchronize()
        return g_raw, xyz2


def _table_launch(sc, pad, layout):
    planes, lines = V.vm_tensors(sc, pad)
    dp, dl = {k: _lay(planes[k], layout) for k in KEYS}, {k: _lay(lines[k], layout) for k in KEYS}
    o, d = (_cuda(a) for a in sc.arrays())
    return (lambda: _Launch(_scene_cfg(sc), dp, dl, o, d)), dp, dl


@pytest.fixture(scope='module')
def restated(oracle):
    """the host restatement of every (scene, padding), computed once"""
    out = {}
    for sc in SCENES:
        for pad in (True, False):
            out[sc.name, pad] = V.cpu_forward_vm(sc, oracle, *V.vm_tensors(sc, pad))[0]
    return out


# ------------------------------------------------------------------------------------------ 1. the case table
@pytest.mark.parametrize('layout', ['cf', 'cl'])
@pytest.mark.parametrize('pad', [True, False], ids=['padded', 'unpadded'])
@pytest.mark.parametrize('sc', SCENES, ids=[s.name for s in SCENES])
def test_edge_case_table(sc, pad, layout, restated):
    launch, dp, dl = _table_launch(sc, pad, layout)
    assert dp['xy'].shape[1] == V.TABLE[sc.name][0 if pad else 1] and (dp['xy'].stride(1) == 1) == (layout == 'cl')
    q = launch()
    want, got = restated[sc.name, pad], q.result
    E = M.check_records(q.R, _np(q.n_steps), sc.thres, _np(q.n3), _np(q.last))
    assert E == V.TABLE[sc.name][3]
    ray_id, step_id, w, a = q.gather()
    assert M.check_gather(q.R, _np(q.n3), _np(q.off3), _np(ray_id), _np(step_id), _np(w), _np(a)) == int(q.off3[-1])
    assert np.array_equal(got.n2, want.n2) and np.array_equal(got.n3, want.n3) and np.array_equal(got.n_steps, want.n_steps)
    assert np.array_equal(got.R.step, want.R.step) and np.array_equal(got.R.flag, want.R.flag)
    for name, target, pred in sc.rows:
        assert pred(got), f'{sc.name}: row {name} ({target}) does not hit its edge on the device'
    again = launch()
    assert all(torch.equal(x, y) for x, y in zip(q.outputs(), again.outputs()))            # byte for byte
    print(sc.name, 'R', dp['xy'].shape[1], layout, 'records', E, 'kept', int(q.off3[-1]))


# ------------------------------------------------------------------------------------------ 2. the bits of the density
def _assert_density_bits(q, planes, lines):
    from directvoxgo_amd import render_utils
    from directvoxgo_amd.ops import vm_density_fwd
    cfg = q.cfg
    raw = vm_density_fwd(planes, lines, q.record_positions(), cfg.xyz_min_t, cfg.xyz_max_t)
    e, a = render_utils.raw2alpha(raw, cfg.act_shift, cfg.interval)
    assert e.shape[0] == q.R.ray.shape[0] > 0
    assert torch.equal(e, _cuda(q.R.exp_d)) and torch.equal(a, _cuda(q.R.alpha))
    return int(e.shape[0])


@pytest.mark.parametrize('layout', ['cf', 'cl'])
@pytest.mark.parametrize('pad', [True, False], ids=['padded', 'unpadded'])
@pytest.mark.parametrize('sc', SCENES, ids=[s.name for s in SCENES])
def test_density_bits_on_the_table(sc, pad, layout):
    launch, dp, dl = _table_launch(sc, pad, layout)
    _assert_density_bits(launch(), dp, dl)


@pytest.fixture(scope='module')
def scene():
    from directvoxgo_amd.scenes import synthetic_scene
    return synthetic_scene(world=32, n_rays=2048, seed=6, device='cuda')


def _rk(sc, **kw):
    return dict(near=sc['near'], far=sc['far'], bg=1, stepsize=0.5, **kw)


def _scene_model(sc, seed=1, **kw):
    """tests/test_gpu_tensorf.py's model, restated: a separable Gaussian blob in component 0 of plane and line xy, 0.01 * randn
    elsewhere, density_offset = -9"""
    from directvoxgo_amd.tensorf import TensoRFVoxGO
    torch.manual_seed(seed)
    m = TensoRFVoxGO(sc['xyz_min'], sc['xyz_max'], **{**dict(
        num_voxels=sc['world'] ** 3, num_voxels_base=sc['world'] ** 3, alpha_init=1e-2, fast_color_thres=1e-4, n_comp=8,
        density_n_comp=4, density_offset=OFFSET, rgbnet_dim=6, rgbnet_width=64), **kw})
    for p in m.rgbnet.parameters():
        torch.nn.init.normal_(p, std=0.1)
    m = m.cuda()
    with torch.no_grad():
        for p in list(m.density_planes.values()) + list(m.density_lines.values()):
            p.mul_(0.1)
        pl, ln = m.density_planes['xy'], m.density_lines['xy']
        ax = [torch.linspace(float(sc['xyz_min'][a]), float(sc['xyz_max'][a]), n, device='cuda')
              for a, n in ((1, pl.shape[2]), (2, pl.shape[3]), (0, ln.shape[2]))]
        pl[0, 0] = AMP * torch.exp(-(ax[0][:, None] ** 2 + ax[1][None, :] ** 2) / SIGMA ** 2)
        ln[0, 0, :, 0] = torch.exp(-ax[2] ** 2 / SIGMA ** 2)
    return m


@pytest.mark.parametrize('R', [3, 4])
def test_density_bits_on_a_random_scene(scene, R):
    sc = scene
    m = _scene_model(sc, density_n_comp=R)
    cfg = m._march_vm_cfg(sc['near'], sc['far'], 0.5)
    dp, dl = {k: m.density_planes[k].detach() for k in KEYS}, {k: m.density_lines[k].detach() for k in KEYS}
    q = _Launch(cfg, dp, dl, sc['rays_o'], sc['rays_d'])
    M.check_records(q.R, _np(q.n_steps), cfg.thres, _np(q.n3), _np(q.last))
    n = _assert_density_bits(q, dp, dl)
    cf = {k: t.contiguous() for k, t in dp.items()}, {k: t.contiguous() for k, t in dl.items()}
    assert cf[0]['xy'].stride(1) != 1 or R == 1
    q2 = _Launch(cfg, *cf, sc['rays_o'], sc['rays_d'])
    assert all(torch.equal(x, y) for x, y in zip(q.outputs(), q2.outputs()))               # the layout changes no bit
    print('R', R, 'records', n, 'rays with records', int((q.n2 > 0).sum()))
    assert n > 1000


# ------------------------------------------------------------------------------------------ 3. the backward kernel
@pytest.mark.parametrize('grads', ['random', 'no_last', 'quiet_rays'])
@pytest.mark.parametrize('sc', SCENES, ids=[s.name for s in SCENES])
def test_backward_kernel_against_the_tree_reference(sc, grads):
    launch, _, _ = _table_launch(sc, True, 'cl')
    q = launch()
    N, M3 = q.N, int(q.off3[-1])
    gen = torch.Generator(device='cuda').manual_seed(3)
    gw = torch.randn(M3, device='cuda', generator=gen)
    gl = None if grads != 'random' else torch.randn(N, device='cuda', generator=gen)
    if grads == 'quiet_rays':                      # every other ray without any upstream gradient: the zero rule
        ray_of = torch.repeat_interleave(torch.arange(N, device='cuda'), q.n3.long())
        gw[ray_of % 2 == 0] = 0
    g_raw, xyz2 = q.backward(gw, gl)
    R = q.R
    O = M.density_bwd_reference(R, _np(q.last), M.gw_per_record(R, _np(q.off3), _np(gw)), None if gl is None else _np(gl),
                                sc.interval, order='tree')
    worst = M.check_density_bwd(R, O, _np(g_raw), 'march_vm_density_bwd')
    assert torch.equal(xyz2, q.record_positions())
    if grads == 'quiet_rays':
        assert O.zero.any() and (~O.zero).any()
    again = q.backward(gw, gl)
    assert torch.equal(g_raw, again[0]) and torch.equal(xyz2, again[1])
    print(sc.name, grads, 'records', R.ray.shape[0], 'worst err / bound', round(worst, 4))


def test_backward_kernel_ray_lengths():
    have = set()
    for sc in SCENES[:2]:
        have |= set(int(v) for v in _np(_table_launch(sc, True, 'cl')[0]().n2))
    assert {1, 63, 64, 65, 129} <= have and max(have) > 512


# ------------------------------------------------------------------------------------------ 4. the scatter
def _check_six(grads, ref, tag):
    """test_gpu_vm_density.check_grads's statement: (n + 12) U A per texel and node, exact zero where nothing contributes"""
    rp, rl = ref
    worst = 0.0
    for k in KEYS:
        for name, dev, (g, Ag, n) in (('plane', grads[k][0], rp[k]), ('line', grads[k + '_line'][0, :, :, 0], rl[k])):
            gg = _np(dev).astype(np.float64)
            assert gg.shape == g.shape
            err, bound = np.abs(gg - g), (n[None] + 12) * VO.U * Ag
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), (tag, k, name, float((err - bound).max()))
            assert (gg[:, n == 0] == 0).all(), (tag, k, name)
    return worst


def _autograd_case(which, scene):
    """-> (cfg, planes, lines as numpy, rays): a table scene (R = 28) or the random scene (R = 4)"""
    if which == 'fine129':
        sc = SCENES[0]
        planes, lines = V.vm_tensors(sc, True)
        o, d = (_cuda(a) for a in sc.arrays())
        return _scene_cfg(sc), planes, lines, o, d
    m = _scene_model(scene)
    return (m._march_vm_cfg(scene['near'], scene['far'], 0.5), {k: _np(m.density_planes[k]) for k in KEYS},
            {k: _np(m.density_lines[k]) for k in KEYS}, scene['rays_o'], scene['rays_d'])


@pytest.mark.parametrize('layout', ['cf', 'cl'])
@pytest.mark.parametrize('which', ['fine129', 'random'])
def test_autograd_scatter_against_the_oracle(which, layout, scene):
    from directvoxgo_amd import fused as F
    cfg, planes, lines, o, d = _autograd_case(which, scene)
    dp = {k: _lay(planes[k], layout).requires_grad_() for k in KEYS}
    dl = {k: _lay(lines[k], layout).requires_grad_() for k in KEYS}
    w, alpha, last, pts, ray_id, step_id, off3 = F.fused_march_vm(dp, dl, o, d, cfg)
    assert pts.shape == (w.shape[0], 3) and off3.shape[0] == o.shape[0] + 1 and not alpha.requires_grad and not pts.requires_grad
    gen = torch.Generator(device='cuda').manual_seed(11)
    gw, gl = torch.randn(w.shape, device='cuda', generator=gen), torch.randn(last.shape, device='cuda', generator=gen)
    mn, mx = _np(cfg.xyz_min_t), _np(cfg.xyz_max_t)
    seen = []
    for _ in range(2):                             # the second call must start from zero-filled buffers of its own
        for t in list(dp.values()) + list(dl.values()):
            t.grad = None
        with _Spy() as spy:
            torch.autograd.backward([w, last], [gw, gl], retain_graph=True)
            torch.cuda.synchronize()
        assert spy.names() == ['dvgo_march_vm_density_bwd', 'dvgo_vm_density_bwd']
        args = spy.calls[1][1]
        g_raw, xyz2 = _np(args[0]), _np(args[-7])
        assert g_raw.ndim == 1 and xyz2.shape == (g_raw.shape[0], 3) and np.isfinite(g_raw).all()
        live = g_raw != 0                          # the scatter passes over exact zeros: they contribute nowhere
        ref = DO.backward(planes, lines, xyz2[live], mn, mx, g_raw[live])
        got = {**{k: dp[k].grad for k in KEYS}, **{k + '_line': dl[k].grad for k in KEYS}}
        assert all(got[k].shape == dp[k].shape and got[k + '_line'].shape == dl[k].shape for k in KEYS)
        worst = _check_six(got, ref, (which, layout))
        seen.append(g_raw)
        print(which, layout, 'records', g_raw.shape[0], 'non-zero', int(live.sum()), 'worst err / bound', round(worst, 4))
    assert np.array_equal(seen[0], seen[1]) and live.sum() > 100


# ------------------------------------------------------------------------------------------ 5. the model
def _pair(sc, **kw):
    from directvoxgo_amd.checkpoint import model_kwargs_of
    from directvoxgo_amd.tensorf import TensoRFVoxGO
    m0 = _scene_model(sc, **kw)
    assert m0.fused_march is False
    m1 = TensoRFVoxGO(**{**model_kwargs_of({'model_kwargs': m0.get_kwargs()}), 'fused_march': True}).cuda()
    m1.load_state_dict(m0.state_dict())
    return m0, m1


@pytest.mark.parametrize('R', [4, 3])
def test_model_paths_agree_bit_for_bit(scene, R):
    sc = scene
    m0, m1 = _pair(sc, density_n_comp=R)
    args = (sc['rays_o'], sc['rays_d'], sc['viewdirs'])
    with torch.no_grad():
        with _Spy() as s0:
            a = m0(*args, render_depth=True, **_rk(sc))
        with _Spy() as s1:
            b = m1(*args, render_depth=True, **_rk(sc))
    assert set(a) == set(b) == {'alphainv_last', 'weights', 'rgb_marched', 'raw_alpha', 'raw_rgb', 'ray_id', 'depth'}
    assert a['ray_id'].shape[0] > 1000
    for k in ('ray_id', 'weights', 'raw_alpha', 'alphainv_last', 'raw_rgb', 'rgb_marched', 'depth'):
        assert torch.equal(a[k], b[k]), k
    sampled = lambda s: [n for n in s.names() if n.startswith('dvgo_sample_pts') or n == 'dvgo_vm_density_fwd']     # noqa: E731
    assert 'dvgo_vm_density_fwd' in sampled(s0) and any(n.startswith('dvgo_sample_pts') for n in sampled(s0))
    assert sampled(s1) == [] and s1.names().count('dvgo_march_vm_density') == 1 and 'dvgo_march_gather' in s1.names()


def test_model_gradients_overrides_and_refusals(scene):
    from directvoxgo_amd.pose import CameraRefiner, refine_poses
    from directvoxgo_amd.scenes import pose_spherical
    from directvoxgo_amd.tensorf import TENSORF_FINE_TRAIN
    sc = scene
    m0, m = _pair(sc)
    args = (sc['rays_o'], sc['rays_d'], sc['viewdirs'])
    res = m(*args, **_rk(sc))
    (res['rgb_marched'] - sc['target']).pow(2).mean().backward()
    every = list(m.density_planes.items()) + list(m.density_lines.items()) + list(m.planes.items()) + list(m.lines.items()) + \
        [('basis', m.basis)] + list(m.rgbnet.named_parameters())
    assert len(every) >= 12 + 1 + 2
    for name, p in every:
        assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), name
        assert float(p.grad.abs().sum()) > 0, name
    # the caller's density tensors are marched instead of the model's own, and take the gradient
    m.zero_grad(set_to_none=True)
    feats = {**{k: p.detach() for k, p in m.planes.items()},
             'xy_density': (m.density_planes['xy'].detach() * 0.5).requires_grad_(),
             'xy_density_line': m.density_lines['xy'].detach().clone().requires_grad_()}
    ext = m.render(feats, *args, **_rk(sc))['rgb_marched']
    with torch.no_grad():
        assert torch.equal(ext, m0.render(feats, *args, **_rk(sc))['rgb_marched']) and not torch.equal(ext, res['rgb_marched'])
    ext.sum().backward()
    assert float(feats['xy_density'].grad.abs().sum()) > 0 and float(feats['xy_density_line'].grad.abs().sum()) > 0
    assert m.density_planes['xy'].grad is None and float(m.density_planes['yz'].grad.abs().sum()) > 0
    # refusals name the class
    with pytest.raises(NotImplementedError, match='TensoRFVoxGO'):
        m(sc['rays_o'].clone().requires_grad_(), sc['rays_d'], sc['viewdirs'], **_rk(sc))
    poses = pose_spherical(20.0, -30.0, 4.0)[None, :3, :4]
    ref = CameraRefiner(poses, [[8, 8]], [np.array([[8.0, 0, 4], [0, 8.0, 4], [0, 0, 1]], np.float32)])
    with pytest.raises(NotImplementedError, match='TensoRFVoxGO'):
        refine_poses(m, ref, torch.zeros(1, 8, 8, 3), TENSORF_FINE_TRAIN, dict(near=0.1, far=1.0, stepsize=0.5, bg=1), 1, 8, 1e-3)


def test_train_steps_and_scale_volume_grid(scene):
    from directvoxgo_amd.tensorf import TENSORF_FINE_TRAIN
    from directvoxgo_amd.train import TrainStep
    sc = scene
    _, m = _pair(sc)
    rk = _rk(sc)
    step = TrainStep(m, dict(TENSORF_FINE_TRAIN), rk)
    assert not step.can_capture() and not m.can_keep_count_on_device()
    args = (sc['rays_o'], sc['rays_d'], sc['viewdirs'], sc['target'])
    with _Spy() as spy:
        losses = [float(step(*args, global_step=s)) for s in (1, 2, 3)]
    print('losses', losses)
    assert losses[2] < losses[0] and spy.names().count('dvgo_march_vm_density') == 3 and 'dvgo_vm_density_fwd' not in spy.names()
    m.scale_volume_grid(40 ** 3)
    ws = tuple(int(v) for v in m.world_size)
    assert min(ws) > 32 and tuple(m.mask_cache.mask.shape) == ws
    with torch.no_grad():
        b = m(*args[:3], render_depth=True, **rk)
    assert torch.isfinite(b['rgb_marched']).all() and b['ray_id'].shape[0] > 0
    assert np.isfinite(float(step(*args, global_step=4)))
