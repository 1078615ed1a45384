"""GPU: the plane regulariser (csrc/plane_tv.hip, ops.plane_reg_add_grad) against the float32 form of
tests/plane_tv_oracle.py bit for bit, on every element of every tensor of a call; its bit tie to the 3-D total-variation
kernel; the model method on VMTriPlaneVoxGO and TriPlaneVoxGO; TrainStep's window, dense flag and weights; and what a dense
plane TV does to texels no sample touched.

The float32 form is within 8 U A of the float64 form on these inputs (tests/test_plane_tv_host.py, which derives the bound);
the kernel has to reproduce the float32 form exactly, -0.0 included, so no tolerance appears here.
"""
import functools

import numpy as np
import pytest
import torch

import plane_tv_oracle as PO

pytestmark = pytest.mark.gpu


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def lay_out(p, layout):
    """numpy [1,C,H,W] -> a device tensor of that shape: channel-first ('cf'), channels-last ('cl'), a channels-last view
    that starts one float off a 16-byte boundary ('off'), or one of two dense layouts that are neither: memory order
    H, C, W ('hcw') and W, H, C ('whc')."""
    t = cu(p)
    _, C, H, W = t.shape
    if layout == 'cf':
        return t
    if layout == 'cl':
        return t.contiguous(memory_format=torch.channels_last)
    if layout == 'hcw':
        view = torch.empty((H, C, W), device='cuda').permute(1, 0, 2).unsqueeze(0)
    elif layout == 'whc':
        view = torch.empty((W, H, C), device='cuda').permute(2, 1, 0).unsqueeze(0)
    else:
        buf = torch.zeros(t.numel() + 1, device='cuda')
        assert buf.data_ptr() % 16 == 0
        view = buf[1:].as_strided((1, C, H, W), (H * W * C, 1, W * C, C))
        assert view.data_ptr() % 16 == 4
    view.copy_(t)
    return view


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def run_and_compare(tensors, layouts, weights, dense):
    """One call over all `tensors` [(param, grad) as numpy [C,H,W]]; every tensor's gradient against reg32, bit for bit,
    and every parameter unchanged."""
    from directvoxgo_amd.ops import plane_reg_add_grad
    dp = [lay_out(p[None], lay) for (p, _), lay in zip(tensors, layouts)]
    dg = [lay_out(g[None], lay) for (_, g), lay in zip(tensors, layouts)]
    plane_reg_add_grad(dp, dg, weights, dense)
    for k, ((p, g), w) in enumerate(zip(tensors, weights)):
        ref = PO.reg32(p, g, *w, dense)
        got = dg[k].cpu().numpy()[0]
        assert got.dtype == ref.dtype == np.float32
        bad = got.view(np.uint32) != ref.view(np.uint32)
        assert not bad.any(), (k, layouts[k], int(bad.sum()), np.argwhere(bad)[:4].tolist())
        assert np.array_equal(bits(dp[k])[0], p.view(np.uint32))
        assert not np.array_equal(got.view(np.uint32), g.view(np.uint32)) or p.shape[1:] == (1, 1)   # (it did something)
    return dp, dg


@functools.lru_cache(maxsize=None)
def six(R):
    return PO.six(R, 100 + R)


# ---------------------------------------------------------------------------------------------- kernel against the oracle
@pytest.mark.parametrize('l1', [False, True])
@pytest.mark.parametrize('dense', [True, False])
@pytest.mark.parametrize('layout', ['cf', 'cl', 'off'])
@pytest.mark.parametrize('R', [1, 3, 16])
def test_six_tensor_call_against_the_float32_oracle(R, layout, dense, l1):
    """Planes (5,7), (6,4), (3,9) and lines 6, 1, 9 in one call, every element of all six."""
    run_and_compare(six(R), [layout] * 6, PO.weights_of(6, l1), dense)


@pytest.mark.parametrize('dense', [True, False])
@pytest.mark.parametrize('layout', ['hcw', 'whc'])
def test_layouts_that_are_neither_channels_last_nor_channel_first(layout, dense):
    """The strided fallback: rows of W elements one column stride apart."""
    run_and_compare(six(3), [layout] * 6, PO.weights_of(6, True), dense)


@pytest.mark.parametrize('dense', [True, False])
def test_rows_longer_than_a_workgroup_and_a_table_that_crosses_tensors(dense):
    """70 x 130 with R = 16, channels-last: a row is 2080 floats, more than eight per thread; a small plane and a line
    behind it in the same launch."""
    run_and_compare(PO.big(7), ['cl'] * 3, PO.weights_of(3, True), dense)


@pytest.mark.parametrize('dense', [True, False])
def test_one_tensor_and_eight_tensors(dense):
    """n_tensors = 1, and 8 with mixed layouts: the six above, a line of 4 nodes and a plane of one row (H == 1)."""
    rng = np.random.default_rng(5)
    eight = six(3) + [PO.tensor(rng, 3, 4, 1), PO.tensor(rng, 3, 1, 5)]
    run_and_compare(eight, ['cl', 'cf', 'off', 'cl', 'cf', 'whc', 'hcw', 'cl'], PO.weights_of(8, True), dense)
    run_and_compare(eight, ['cf', 'cl', 'hcw', 'off', 'cl', 'cf', 'cl', 'cf'], PO.weights_of(8, False), dense)
    for layout in ('cf', 'cl'):
        run_and_compare(six(16)[:1], [layout], [(0.4, 0.6, -0.02)], dense)
        run_and_compare(six(16)[4:5], [layout], [(0.4, 0.6, 0.02)], dense)          # the line of one node alone
    from directvoxgo_amd.ops import plane_reg_add_grad
    nine = [torch.zeros(1, 2, 3, 3, device='cuda') for _ in range(9)]
    with pytest.raises(RuntimeError, match='invalid argument'):
        plane_reg_add_grad(nine, [torch.zeros_like(t) for t in nine], [(0.1, 0.1, 0.0)] * 9, dense)


def test_repeatable_and_refuses_mismatched_strides():
    from directvoxgo_amd.ops import plane_reg_add_grad
    a = run_and_compare(six(16), ['cl'] * 6, PO.weights_of(6, True), True)[1]
    b = run_and_compare(six(16), ['cl'] * 6, PO.weights_of(6, True), True)[1]
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))
    p, g = six(16)[0]
    with pytest.raises(RuntimeError, match='share strides'):
        plane_reg_add_grad([lay_out(p[None], 'cl')], [lay_out(g[None], 'cf')], [(0.1, 0.1, 0.0)], True)


# ---------------------------------------------------------------------------------------------- tie to the 3-D kernel
@pytest.mark.parametrize('dense', [True, False])
@pytest.mark.parametrize('layout', ['cf', 'cl', 'off'])
@pytest.mark.parametrize('R', [1, 3, 16])
def test_bit_equal_to_the_3d_kernel_on_a_one_slice_view(R, layout, dense):
    """wl1 = 0, wh = ww = 0.75 against ops.total_variation_add_grad(wy = wz = 4.5) on the same memory viewed as
    [1,C,1,H,W]: 4.5 / 6 is exactly 0.75 in float32, the i axis of size 1 adds nothing, the term order is the same."""
    from directvoxgo_amd.ops import plane_reg_add_grad, total_variation_add_grad
    dp = [lay_out(p[None], layout) for p, _ in six(R)]
    ours = [lay_out(g[None], layout) for _, g in six(R)]
    theirs = [lay_out(g[None], layout) for _, g in six(R)]
    plane_reg_add_grad(dp, ours, [(0.75, 0.75, 0.0)] * 6, dense)
    for p, g in zip(dp, theirs):
        total_variation_add_grad(p.unsqueeze(2), g.unsqueeze(2), 4.5, 4.5, 4.5, dense)
    for a, b, (_, g0) in zip(ours, theirs, six(R)):
        assert np.array_equal(bits(a), bits(b))
        assert not np.array_equal(bits(a)[0], g0.view(np.uint32)) or g0.shape[1:] == (1, 1)


# ---------------------------------------------------------------------------------------------- the models
class _Calls:
    """names of the library calls issued inside, in order"""

    def __enter__(self):
        from directvoxgo_amd import _lib
        self._L, self._orig, self.names = _lib, _lib.call, []

        def call(name, *args):
            self.names.append(name)
            return self._orig(name, *args)
        _lib.call = call
        return self

    def __exit__(self, *exc):
        self._L.call = self._orig
        return False


@pytest.fixture(scope='module')
def scene():
    from directvoxgo_amd.scenes import synthetic_scene
    return synthetic_scene(world=24, n_rays=1024, seed=6, device='cuda')


COMMON = dict(alpha_init=1e-2, fast_color_thres=1e-4, rgbnet_dim=6, rgbnet_width=64)


def _model(sc, cls, seed=1, **kw):
    torch.manual_seed(seed)
    m = cls(sc['xyz_min'], sc['xyz_max'], num_voxels=sc['world'] ** 3, num_voxels_base=sc['world'] ** 3, **{**COMMON, **kw})
    for p in m.rgbnet.parameters():
        torch.nn.init.normal_(p, std=0.1)
    m = m.cuda()
    with torch.no_grad():
        m.density.copy_(sc['density']); m.mask_cache.mask.copy_(sc['mask'])
        for p in m.planes.values():                       # (the base's planes start at zero: give the stencil something)
            p.copy_(0.8 * torch.randn_like(p))
    return m


def _backward(m, sc):
    rk = dict(near=sc['near'], far=sc['far'], bg=1, stepsize=0.5)
    out = m(sc['rays_o'], sc['rays_d'], sc['viewdirs'], **rk)
    (out['rgb_marched'] - sc['target']).pow(2).mean().backward()


def _expect(p, g, w, dense):
    return PO.reg32(p.detach().cpu().numpy()[0], g.cpu().numpy()[0], *w, dense)


@pytest.mark.parametrize('dense', [True, False])
def test_vm_model_method_is_one_launch_with_the_oracles_values(scene, dense):
    from directvoxgo_amd.vm import VMTriPlaneVoxGO
    m = _model(scene, VMTriPlaneVoxGO, n_comp=8)
    _backward(m, scene)
    tensors = [m.planes[k] for k in PO.KEYS] + [m.lines[k] for k in PO.KEYS]
    before = [t.grad.clone() for t in tensors]
    assert all(float(g.abs().sum()) > 0 for g in before) and any(bool((g == 0).any()) for g in before)
    wp, wl, l1 = 3e-3, 2e-3, 5e-4
    with _Calls() as calls:
        m.plane_regularizers_add_grad(dense, weight_tv_planes=wp, weight_tv_lines=wl, weight_l1_lines=l1)
    assert calls.names == ['dvgo_plane_reg_add_grad']
    for i, (t, g0) in enumerate(zip(tensors, before)):
        H, W = t.shape[2:]
        w = (wp * max(H, W) / 128 / 4,) * 2 + (0.0,) if i < 3 else (wl * H / 128 / 2, 0.0, l1)
        ref = _expect(t, g0, w, dense)
        assert t.grad.stride() == t.stride()
        assert np.array_equal(bits(t.grad)[0], ref.view(np.uint32)), i
        assert not np.array_equal(bits(t.grad), bits(g0)), i
    # planes only: three tensors, still one call; the lines' gradients stay as they are
    held = [t.grad.clone() for t in tensors[3:]]
    with _Calls() as calls:
        m.plane_regularizers_add_grad(dense, weight_tv_planes=wp)
    assert calls.names == ['dvgo_plane_reg_add_grad'] and all(torch.equal(t.grad, h) for t, h in zip(tensors[3:], held))
    with _Calls() as calls:                                # all weights zero: nothing is launched
        m.plane_regularizers_add_grad(dense)
    assert calls.names == []


def test_missing_gradients_are_skipped_or_created(scene):
    from directvoxgo_amd.vm import VMTriPlaneVoxGO
    m = _model(scene, VMTriPlaneVoxGO, n_comp=4)
    tensors = [m.planes[k] for k in PO.KEYS] + [m.lines[k] for k in PO.KEYS]
    with _Calls() as calls:
        m.plane_regularizers_add_grad(False, weight_tv_planes=1e-2, weight_tv_lines=1e-2, weight_l1_lines=1e-3)
    assert calls.names == [] and all(t.grad is None for t in tensors)          # sparse: no gradient, nothing to touch
    with _Calls() as calls:
        m.plane_regularizers_add_grad(True, weight_tv_planes=1e-2, weight_tv_lines=1e-2, weight_l1_lines=1e-3)
    assert calls.names == ['dvgo_plane_reg_add_grad']
    for i, t in enumerate(tensors):
        H, W = t.shape[2:]
        w = (1e-2 * max(H, W) / 128 / 4,) * 2 + (0.0,) if i < 3 else (1e-2 * H / 128 / 2, 0.0, 1e-3)
        assert t.grad.stride() == t.stride()
        assert np.array_equal(bits(t.grad)[0], _expect(t, torch.zeros_like(t), w, True).view(np.uint32)), i
    feats = {k: p.detach().clone().requires_grad_() for k, p in m.planes.items()}          # the caller's planes stay theirs
    m.render(feats, scene['rays_o'], scene['rays_d'], scene['viewdirs'], near=scene['near'], far=scene['far'], bg=1,
             stepsize=0.5)['rgb_marched'].sum().backward()
    kept = {k: f.grad.clone() for k, f in feats.items()}
    m.plane_regularizers_add_grad(True, weight_tv_planes=1e-2)
    assert all(torch.equal(feats[k].grad, kept[k]) for k in feats)


@pytest.mark.parametrize('dense', [True, False])
def test_triplane_model_method(scene, dense):
    from directvoxgo_amd.triplane import TriPlaneVoxGO
    m = _model(scene, TriPlaneVoxGO)
    _backward(m, scene)
    before = {k: m.planes[k].grad.clone() for k in PO.KEYS}
    with _Calls() as calls:
        m.plane_regularizers_add_grad(dense, weight_tv_planes=4e-3)
    assert calls.names == ['dvgo_plane_reg_add_grad']
    for k in PO.KEYS:
        p = m.planes[k]
        w = 4e-3 * max(p.shape[2:]) / 128 / 4
        assert np.array_equal(bits(p.grad)[0], _expect(p, before[k], (w, w, 0.0), dense).view(np.uint32)), k
        assert not np.array_equal(bits(p.grad), bits(before[k]))
    with pytest.raises(ValueError, match='no lines'):
        m.plane_regularizers_add_grad(dense, weight_tv_lines=1e-3)


# ---------------------------------------------------------------------------------------------- training
def test_train_step_window_dense_flag_and_weights(scene):
    """tv_after = 0, tv_before = 3, tv_every = 1, tv_dense_before = 2: the method runs at steps 1 and 2 only, dense at step 1
    and not at step 2, with every weight divided by the global ray count; one library call each time."""
    from directvoxgo_amd.train import TrainStep
    from directvoxgo_amd.vm import VM_FINE_TRAIN, VMTriPlaneVoxGO
    sc = scene
    m = _model(sc, VMTriPlaneVoxGO, n_comp=8)
    cfg = dict(VM_FINE_TRAIN, tv_after=0, tv_before=3, tv_every=1, tv_dense_before=2, weight_tv_planes=0.5, weight_tv_lines=0.25,
               weight_l1_lines=0.125)
    step = TrainStep(m, cfg, dict(near=sc['near'], far=sc['far'], bg=1, stepsize=0.5))
    assert not step.can_capture()
    seen, inner = [], m.plane_regularizers_add_grad

    def record(dense_mode, **weights):
        with _Calls() as calls:
            inner(dense_mode, **weights)
        seen.append((now[0], dense_mode, weights, calls.names))
    m.plane_regularizers_add_grad = record
    now = [0]
    args = (sc['rays_o'], sc['rays_d'], sc['viewdirs'], sc['target'])
    for s in (1, 2, 3, 4):
        now[0] = s
        assert torch.isfinite(step(*args, global_step=s))
    n = sc['rays_o'].shape[0]
    want = dict(weight_tv_planes=0.5 / n, weight_tv_lines=0.25 / n, weight_l1_lines=0.125 / n)
    assert seen == [(1, True, want, ['dvgo_plane_reg_add_grad']), (2, False, want, ['dvgo_plane_reg_add_grad'])]


# ---------------------------------------------------------------------------------------------- behaviour
def test_dense_plane_tv_moves_texels_no_sample_touched(scene):
    """Rays parallel to -z through one corner of the box's xy square, marched over the top of the box only: their samples
    lie in one corner, so most texels of every plane get an exactly zero gradient.  One step (plain Adam on the planes: a
    zero gradient is a zero update) leaves those texels bit-identical without the keys and with a sparse plane TV; a dense
    plane TV moves them."""
    from directvoxgo_amd.train import TrainStep
    from directvoxgo_amd.vm import VM_FINE_TRAIN, VMTriPlaneVoxGO
    sc = scene
    mn, mx = sc['xyz_min'].cpu(), sc['xyz_max'].cpu()
    ext = mx - mn
    gen = torch.Generator().manual_seed(3)
    N = 512
    o = torch.empty(N, 3)
    o[:, :2] = mx[:2] - 0.3 * ext[:2] * torch.rand(N, 2, generator=gen) - 0.01 * ext[:2]
    o[:, 2] = mx[2] + 1.0
    d = torch.tensor([[0.0, 0.0, -1.0]]).repeat(N, 1)
    o, d = o.cuda(), d.cuda()
    target = torch.rand(N, 3, generator=gen).cuda()
    rk = dict(near=1.0, far=1.0 + 0.3 * float(ext[2]), bg=1, stepsize=0.5)
    window = dict(tv_after=0, tv_before=3, tv_every=1)
    runs = {'none': dict(VM_FINE_TRAIN, **window, tv_dense_before=2),
            'dense': dict(VM_FINE_TRAIN, **window, tv_dense_before=2, weight_tv_planes=1.0),
            'sparse': dict(VM_FINE_TRAIN, **window, tv_dense_before=0, weight_tv_planes=1.0)}
    after, grads = {}, {}
    for name, cfg in runs.items():
        m = _model(sc, VMTriPlaneVoxGO, n_comp=4)
        with torch.no_grad():
            m.density.zero_(); m.mask_cache.mask.fill_(True)          # every sample in the marched span survives
        init = {k: p.detach().clone() for k, p in m.planes.items()}
        TrainStep(m, cfg, rk)(o, d.clone(), d.clone(), target, global_step=1)
        after[name] = {k: p.detach().clone() for k, p in m.planes.items()}
        grads[name] = {k: p.grad.clone() for k, p in m.planes.items()}
    for k in PO.KEYS:
        untouched = grads['none'][k] == 0
        assert 0.5 < float(untouched.float().mean()) < 1.0, k                      # one corner only, but that corner is seen
        same = lambda a, b: np.array_equal(bits(a[untouched]), bits(b[untouched]))  # noqa: E731
        assert same(after['none'][k], init[k]) and same(after['sparse'][k], init[k]), k
        assert not torch.equal(after['sparse'][k], after['none'][k]), k            # (the sparse TV did act, on touched texels)
        moved = after['dense'][k][untouched] != init[k][untouched]
        assert float(moved.float().mean()) > 0.9, k
