"""CPU: the bilinear plane decoder's oracle (tests/interp_oracle.py) pinned against the reference's own interpolate
(tests/golden/make_golden_interp.py) and against the tri-plane sampler's oracle, the argument validation of the two entry
points without a device, and the host side of InterpTriPlaneVoxGO: constructor errors and accepted options, state_dict
keys, kwargs, optimiser groups."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

from conftest import load_golden

import interp_oracle as IO
import triplane_oracle as TO

CASES = [(agg, cell) for agg in ('concat', 'sum') for cell in (True, False)]
INTERP = ('interp_xy', 'interp_yz', 'interp_zx')


def fixture_nets(z, cell, C, P, dtype=torch.float64):
    """The fixture's three Interp_MLPs, loaded by their reference names with strict=True, as one module."""
    from directvoxgo_amd.liif import InterpMLP
    holder = torch.nn.Module()
    for net in INTERP:
        setattr(holder, net, InterpMLP(C + 2 + 4 * P + (2 if cell else 0), C, width=8, depth=3))
    prefix = f'c{int(cell)}_sd_'
    holder.load_state_dict({k[len(prefix):]: torch.from_numpy(v) for k, v in z.items() if k.startswith(prefix)}, strict=True)
    return holder.to(dtype).eval()


def test_fma32_is_correctly_rounded():
    """Against exact rational arithmetic, on random operands and on sums that fall on a float32 tie broken by the
    product's low bits (where rounding the float64 sum a second time would go wrong)."""
    rng = np.random.default_rng(3)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = (rng.standard_normal(4000) * 10.0 ** rng.integers(-8, 3, 4000)).astype(np.float32)
    a[:4] = np.float32(1 + 2.0 ** -23); b[:4] = np.float32(1 + 2.0 ** -23)             # product 1 + 2^-22 + 2^-46
    c[:4] = np.array([2.0 ** 29 + 2.0 ** 5, 2.0 ** 30, -2.0 ** 24, 2.0 ** 24], np.float32)
    a[4] = np.float32(2.0 ** -30); b[4] = np.float32(2.0 ** -30); c[4] = np.float32(1 + 2.0 ** -23)
    a[5] = np.float32(3 * 2.0 ** -30); b[5] = np.float32(2.0 ** -26); c[5] = np.float32(1.0)
    got = IO.fma32(a, b, c)
    assert got.dtype == np.float32
    for x, y, zc, r in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(zc))
        lo, hi = np.nextafter(r, np.float32(-np.inf)), np.nextafter(r, np.float32(np.inf))
        err = abs(Fraction(float(r)) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact), (x, y, zc, r)
        if err == abs(Fraction(float(lo)) - exact) or err == abs(Fraction(float(hi)) - exact):
            assert int(np.float32(r).view(np.uint32)) & 1 == 0, (x, y, zc, r)             # a tie goes to even


@pytest.mark.parametrize('agg, cell', CASES)
def test_oracle_reproduces_the_reference_decoder(agg, cell):
    """Every point of the fixture: the oracle's float32 rows through the fixture's reference MLPs in float32 give
    interp.npz's values at rtol 1e-5 / atol 1e-6; the float64 decoder on the same rows gives them too, and its gradients
    (planes, Interp_MLP parameters) match the reference's at rtol 1e-4 / atol 1e-6."""
    z = load_golden('interp')
    C, P = z['plane_xy'].shape[1], int(z['posbase_pe'])
    p = f'{agg}_c{int(cell)}_'
    planes_np = {k: z['plane_' + k] for k in IO.KEYS}
    inp = IO.rows(planes_np, z['xyz'], z['xyz_min'], z['xyz_max'], z['world_size'], P, cell)
    cols, D = IO.columns(C, P, cell)
    assert inp.shape == (3, 400, D) and inp.dtype == np.float32
    n32 = fixture_nets(z, cell, C, P, torch.float32)
    with torch.no_grad():
        pred = [getattr(n32, 'interp_' + IO.NET_OF[k])(torch.from_numpy(inp[s])).numpy() for s, k in enumerate(IO.KEYS)]
    val32 = np.concatenate(pred, 1) if agg == 'concat' else (pred[0] + pred[1]) + pred[2]
    assert val32.shape == z[p + 'out'].shape == (400, 3 * C if agg == 'concat' else C)
    print('worst |err|', np.abs(val32 - z[p + 'out']).max(), 'at values up to', np.abs(z[p + 'out']).max())
    np.testing.assert_allclose(val32, z[p + 'out'], rtol=1e-5, atol=1e-6)

    nets = fixture_nets(z, cell, C, P)
    planes = {k: torch.from_numpy(z['plane_' + k]).double().requires_grad_() for k in IO.KEYS}
    val = IO.decode(planes, {'xy': nets.interp_xy, 'yz': nets.interp_yz}, z['xyz'], z['xyz_min'], z['xyz_max'],
                    z['world_size'], P, cell, agg)
    np.testing.assert_allclose(val.detach().numpy(), z[p + 'out'], rtol=1e-5, atol=1e-6)
    val.backward(torch.from_numpy(z[agg + '_gout']).double())
    for k in IO.KEYS:
        np.testing.assert_allclose(planes[k].grad.numpy(), z[f'{p}gplane_{k}'], rtol=1e-4, atol=1e-6)
    for name, q in nets.named_parameters():
        if name.startswith('interp_zx.'):
            assert q.grad is None and f'{p}g_{name}' not in z           # built, stored, never used: no gradient
        else:
            np.testing.assert_allclose(q.grad.numpy(), z[f'{p}g_{name}'], rtol=1e-4, atol=1e-6)


def test_fixture_covers_the_edge_cases():
    """Box corners, texel centres, points outside on both sides of every axis, a plane axis of size 1, a non-cubic
    world_size, both cell_decode settings; inside the box q is the normalised coordinate pair."""
    z = load_golden('interp')
    mn, mx, xyz, ws = z['xyz_min'], z['xyz_max'], z['xyz'], z['world_size']
    assert len(set(ws.tolist())) > 1 and z['plane_zx'].shape[3] == 1 and xyz.shape == (400, 3)
    assert (xyz < mn).any(0).all() and (xyz > mx).any(0).all()
    corners = {tuple(np.float32([(mn, mx)[(i >> a) & 1][a] for a in range(3)])) for i in range(8)}
    assert corners <= {tuple(r) for r in xyz}
    assert any(k.endswith('_c0_out') for k in z) and any(k.endswith('_c1_out') for k in z)
    inside = ((xyz >= mn) & (xyz <= mx)).all(1)
    n = ((xyz - mn) / (mx - mn)) * 2 - 1
    for key in IO.KEYS:
        H, W = z['plane_' + key].shape[2:]
        ah, aw = TO.AXES[key]
        ih, iw, w, ok = TO.corners(key, H, W, xyz, mn, mx)
        assert (w[:, ok.all(0)].max(0) == 1).any() or W == 1                 # a sample on a texel centre
        q0, q1 = IO.coord(key, xyz, mn, mx, ws)
        np.testing.assert_allclose(q0[inside], n[inside, aw], atol=1e-6)
        np.testing.assert_allclose(q1[inside], n[inside, ah], atol=1e-6)


@pytest.mark.parametrize('C', [1, 5])
def test_feat_columns_are_the_triplane_oracles(C):
    """The float64 rows' feat columns are tests/triplane_oracle.py's 'concat' value bit for bit (the same corner weights,
    the same sum); the float32 rows' are the four-term fma chain on the same terms: within (4 + 1) u A of it, the bound
    tests/test_gpu_triplane.py holds the kernel to."""
    rng = np.random.default_rng(40 + C)
    mn, mx = np.array([-1.0, -0.8, -0.6], np.float32), np.array([0.9, 1.1, 0.7], np.float32)
    sizes = {'xy': (6, 7), 'yz': (3, 9), 'zx': (8, 1)}
    planes = {k: rng.standard_normal((1, C, *hw)).astype(np.float32) for k, hw in sizes.items()}
    xyz = (rng.random((300, 3)) * (mx - mn) * 1.1 + mn - 0.05 * (mx - mn)).astype(np.float32)
    exp, A = TO.forward(planes, xyz, mn, mx, 'concat')
    r64 = IO.rows(planes, xyz, mn, mx, (4, 9, 2), 3, True, np.float64)
    r32 = IO.rows(planes, xyz, mn, mx, (4, 9, 2), 3, True)
    got64 = np.concatenate([r64[s][:, :C] for s in range(3)], 1)
    got32 = np.concatenate([r32[s][:, :C] for s in range(3)], 1)
    assert got64.dtype == np.float64 and np.array_equal(got64.view(np.uint64), exp.view(np.uint64))
    assert got32.dtype == np.float32 and (np.abs(got32.astype(np.float64) - exp) <= 5 * IO.U * A).all()
    cols, D = IO.columns(C, 3, True)
    for k in ('q', 'cell'):                                   # float32 numbers in both
        assert np.array_equal(r64[..., cols[k]], r32[..., cols[k]].astype(np.float64))
    assert (np.abs(r32[..., cols['sin']] - r64[..., cols['sin']]) <= IO.U).all()


def test_a_point_with_every_corner_outside():
    """feat = 0, q = 0, so sin = 0 and cos = 1; the cells stay.  Far outside on every axis, and just beyond the last
    texel (more than one cell outside) of each plane and table."""
    mn, mx = -np.ones(3, np.float32), np.ones(3, np.float32)
    planes = {k: np.ones((1, 3, 4, 5), np.float32) for k in IO.KEYS}
    xyz = np.array([[5, -7, 9], [-1.8, 1.8, -1.8], [1e30, -1e30, 1e30]], np.float32)
    P, ws = 3, (4, 5, 6)
    cols, D = IO.columns(3, P, True)
    for dtype in (np.float32, np.float64):
        r = IO.rows(planes, xyz, mn, mx, ws, P, True, dtype)
        assert r.shape == (3, 3, D)
        assert (r[..., cols['feat']] == 0).all() and (r[..., cols['q']] == 0).all()
        assert (r[..., cols['sin']] == 0).all() and (r[..., cols['cos']] == 1).all()
        for s, (ia, ib) in enumerate(IO.TABLE[k] for k in IO.KEYS):
            assert (r[s][:, cols['cell']] == np.array([np.float32(1) / np.float32(ws[ia]), np.float32(1) / np.float32(ws[ib])])).all()
    on = IO.rows(planes, np.zeros((1, 3), np.float32), mn, mx, ws, P, False)        # the centre: feat = 1, q = 0 to rounding
    assert np.allclose(on[..., :3], 1) and on.shape == (3, 1, D - 2) and (np.abs(on[..., 3:5]) <= 2 * IO.U).all()


# ---------------------------------------------------------------------------------------------- entry points
@pytest.fixture(scope='module')
def lib():
    from directvoxgo_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


ONE = ctypes.c_void_p(16)         # any non-null value: rejected before it could be dereferenced, or never reached
PTRS = IO.KEYS + ('xyz', 'mn', 'mx', 'io')


def _rows(lib, name, M=8, C=4, sizes=((6, 7), (3, 9), (8, 2)), null=(), run=0, ws=(13, 13, 9), P=2, cell=1):
    ptr = lambda k: None if k in null else ONE         # noqa: E731
    planes = []
    for k, (H, W) in zip(IO.KEYS, sizes):
        planes += [ptr(k), H, W, 1, W * C, C]
    tail = [C, ptr('xyz'), ptr('mn'), ptr('mx'), M, *ws, P, cell]
    if name == 'dvgo_plane_rows_fwd':
        return getattr(lib, name)(*planes, *tail, ptr('io'), None)
    return getattr(lib, name)(ptr('io'), *planes, *tail, run, None)


@pytest.mark.parametrize('name', ['dvgo_plane_rows_fwd', 'dvgo_plane_rows_bwd'])
def test_entries_validate_before_any_launch(lib, name):
    assert _rows(lib, name, M=0) == 0 and _rows(lib, name, C=0) == 0                # no-ops, pointers not looked at
    assert _rows(lib, name, M=0, null=PTRS) == 0
    assert _rows(lib, name, M=-1) == -1 and _rows(lib, name, C=-1) == -1
    assert _rows(lib, name, P=0) == -1 and _rows(lib, name, P=-3) == -1 and _rows(lib, name, P=0, M=0) == -1
    for k in PTRS:
        assert _rows(lib, name, null=(k,)) == -1, k
    assert _rows(lib, name, sizes=((6, 7), (0, 9), (8, 2))) == -1                   # a plane axis below 1
    assert _rows(lib, name, sizes=((6, 7), (3, 9), (8, -2))) == -1
    for ws in ((0, 13, 9), (13, -1, 9), (13, 13, 0)):                               # a world extent below 1
        assert _rows(lib, name, ws=ws) == -1
    big = (1 << 31) // (3 * 16) + 1                                                 # 3 M D >= 2^31 at C = 4, P = 2, D = 16
    assert _rows(lib, name, M=big) == -2 and _rows(lib, name, M=big - 1, null=('xyz',)) == -1
    assert _rows(lib, name, M=big, cell=0, null=('xyz',)) == -1                     # D = 14: in range again
    assert _rows(lib, name, M=big, C=0) == 0
    assert _rows(lib, name, M=1, P=1 << 29) == -2                                   # a row alone past 2^31
    if name == 'dvgo_plane_rows_bwd':
        assert _rows(lib, name, run=-1) == -1


def test_ops_reject_cpu_tensors_and_bad_arguments():
    from directvoxgo_amd.ops import interp_decode, plane_rows
    planes = {k: torch.zeros(1, 4, 5, 6) for k in IO.KEYS}
    xyz, mn, mx = torch.zeros(7, 3), -torch.ones(3), torch.ones(3)
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        plane_rows(planes, xyz, mn, mx, (8, 8, 8), 2)
    with pytest.raises(ValueError, match='three'):
        plane_rows([planes['xy']] * 2, xyz, mn, mx, (8, 8, 8), 2)
    with pytest.raises(ValueError, match='aggregation'):
        interp_decode(planes, {}, xyz, mn, mx, (8, 8, 8), 2, True, 'mean')


# ---------------------------------------------------------------------------------------------- model, host side
BASE = dict(num_voxels=10 * 12 * 14, num_voxels_base=16 ** 3, alpha_init=1e-2, fast_color_thres=1e-4, posbase_pe=2)
BOX = ([-1.0, -1.2, -1.4], [1.0, 1.2, 1.4])
# configs/nerf/tri_multiscene.py: fine_model_and_render without the encoder's keys (name, pretrained_state_dict, map_depth, ...)
TRI_MULTISCENE = dict(implicit_voxel_feat=True, feat_unfold=False, cell_decode=True, local_ensemble=True, rgbnet_dim=64,
                      posbase_pe=5, rgbnet_depth=3, global_cell_decode=False, no_voxel_feat=False, cat_posemb=True,
                      interp_width=128, interp_depth=3, tri_aggregation='sum', liif=False, feat_pe=0, feat_fourier=False)


def _model(**kw):
    from directvoxgo_amd.interp import InterpTriPlaneVoxGO
    return InterpTriPlaneVoxGO(*BOX, **{**BASE, **kw})


def _interp_keys(depth):
    layers = ['model.0'] + [f'model.{i}.0' for i in range(2, depth)] + [f'model.{depth}']
    return {f'{net}.{layer}.{wb}' for net in INTERP for layer in layers for wb in ('weight', 'bias')}


def test_tri_multiscene_options_state_dict_and_kwargs():
    from directvoxgo_amd.checkpoint import model_kwargs_of
    from directvoxgo_amd.triplane import TriPlaneVoxGO
    m = _model(**TRI_MULTISCENE)
    assert isinstance(m, TriPlaneVoxGO) and not hasattr(m, 'k0') and m.cell_decode and m.cat_posemb and m.posbase_pe == 5
    assert not hasattr(m, 'local_ensemble')
    base = {'xyz_min', 'xyz_max', 'density', 'viewfreq', 'posfreq', 'planes.xy', 'planes.yz', 'planes.zx', 'rgbnet.0.weight',
            'rgbnet.0.bias', 'rgbnet.2.0.weight', 'rgbnet.2.0.bias', 'rgbnet.3.weight', 'rgbnet.3.bias', 'mask_cache.mask',
            'mask_cache.xyz2ijk_scale', 'mask_cache.xyz2ijk_shift'}
    assert set(m.state_dict()) == base | _interp_keys(3)
    assert m.interp_xy.model[0].in_features == 64 + 2 + 4 * 5 + 2 == 88 and m.interp_xy.model[3].out_features == 64
    assert m.interp_xy.model[2][1].p == 0.1 and m.posfreq.tolist() == [1, 2, 4, 8, 16]
    assert m.rgbnet[0].in_features == 64 - 3 + 27 + (3 + 3 * 5 * 2)              # 'sum': feat_dim = rgbnet_dim; cat_posemb
    kw = m.get_kwargs()
    assert kw['implicit_voxel_feat'] is True and kw['liif'] is False and kw['cell_decode'] is True and kw['cat_posemb'] is True
    assert kw['interp_width'] == 128 and kw['interp_depth'] == 3 and kw['interp_dropout'] == 0.1 and kw['posbase_pe'] == 5
    assert kw['tri_aggregation'] == 'sum' and 'local_ensemble' not in kw
    m2 = type(m)(**model_kwargs_of({'model_kwargs': kw}))
    assert set(m2.state_dict()) == set(m.state_dict()) and m2.get_kwargs().keys() == kw.keys()
    assert all(m2.state_dict()[k].shape == v.shape for k, v in m.state_dict().items())


def test_state_dict_keys_are_the_reference_models():
    """The key set of the reference model the fixture was rendered with, but for the image encoder and its Mapping network
    (`encoder.*`, `map.*`: not part of this model) and the model's own planes, which stand in for what they emit; the
    decoders and the colour head load by name."""
    z = load_golden('forward_interp')
    m = _model(rgbnet_dim=4, interp_width=16, interp_depth=3, rgbnet_width=64, tri_aggregation='sum', posbase_pe=2, cat_posemb=True)
    ref = {k for k in z['ref_keys'].tolist() if not k.startswith(('encoder.', 'map.'))}
    assert len(ref) < len(z['ref_keys']) and 'posfreq' in ref and 'interp_zx.model.0.weight' in ref
    ours = set(m.state_dict())
    assert ours - {'planes.xy', 'planes.yz', 'planes.zx'} == ref, (ours ^ ref)
    sd = {k[len('sd_'):]: torch.from_numpy(v) for k, v in z.items() if k.startswith('sd_')}
    assert set(sd) == {k for k in m.state_dict() if k.startswith(('interp_', 'rgbnet.'))}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and not [k for k in missing if k.startswith(('interp_', 'rgbnet.'))]
    assert torch.equal(m.interp_zx.model[3].bias, sd['interp_zx.model.3.bias'])


def test_accepted_options():
    m = _model(rgbnet_dim=4, cell_decode=False, local_ensemble=False, interp_width=16, interp_depth=2, interp_dropout=0.0, posbase_pe=1)
    assert m.interp_yz.model[0].in_features == 4 + 2 + 4 and set(m.state_dict()) >= _interp_keys(2)
    assert m.feat_dim == 12 and m.rgbnet[0].in_features == 12 - 3 + 27 and m.posfreq.tolist() == [1]
    p = _model(rgbnet_dim=4, posbase_pe=4, cat_posemb=True)                       # lib/tri_dvgo.py:212-223
    assert p.rgbnet[0].in_features == 12 - 3 + 27 + (3 + 3 * 4 * 2) and p.interp_xy.model[0].in_features == 4 + 2 + 16 + 2
    d = _model(rgbnet_dim=4, rgbnet_direct=True, tri_aggregation='sum')
    assert d.rgbnet[0].in_features == 4 + 27 and d.posbase_pe == 2
    assert not m.can_keep_count_on_device() and not m.uses_posenc


def test_posbase_pe_zero_is_a_value_error():
    from directvoxgo_amd.interp import InterpTriPlaneVoxGO
    with pytest.raises(ValueError, match='posfreq'):
        _model(rgbnet_dim=4, posbase_pe=0)
    no_key = {k: v for k, v in BASE.items() if k != 'posbase_pe'}
    with pytest.raises(ValueError, match='posfreq'):          # the reference's default is 0: the same error, no silent 5
        InterpTriPlaneVoxGO(*BOX, rgbnet_dim=4, **no_key)
    with pytest.raises(ValueError, match='interp_depth'):
        _model(rgbnet_dim=4, interp_depth=1)


@pytest.mark.parametrize('kw, match', [
    (dict(feat_unfold=True), 'feat_unfold'), (dict(liif=True), 'LIIFTriPlaneVoxGO'), (dict(implicit_voxel_feat=False), 'TriPlaneVoxGO'),
    (dict(global_cell_decode=True), 'global_cell_decode'), (dict(feat_fourier=True), 'feat_fourier'), (dict(feat_pe=4), 'feat_pe'),
    (dict(no_voxel_feat=True), 'no_voxel_feat'), (dict(rgbnet_full_implicit=True), 'rgbnet_full_implicit'),
    (dict(name='edsr-baseline'), 'encoder'), (dict(pretrained_state_dict='x.pth'), 'encoder'), (dict(map_depth=5), 'encoder'),
    (dict(rgbnet_dim=0), 'rgbnet_dim')])
def test_left_out_options_raise_with_their_reason(kw, match):
    with pytest.raises(NotImplementedError, match=match):
        _model(**{'rgbnet_dim': 4, **kw})


def test_the_other_classes_still_reject_this_path():
    from directvoxgo_amd.liif import LIIFTriPlaneVoxGO
    from directvoxgo_amd.triplane import TriPlaneVoxGO
    with pytest.raises(NotImplementedError, match='InterpTriPlaneVoxGO'):
        LIIFTriPlaneVoxGO(*BOX, **{**BASE, 'rgbnet_dim': 4, 'posbase_pe': 0, 'liif': False})
    with pytest.raises(NotImplementedError):
        TriPlaneVoxGO(*BOX, **{**BASE, 'rgbnet_dim': 4, 'posbase_pe': 0, 'implicit_voxel_feat': True, 'liif': False})


def test_left_out_methods_and_data_parallel_raise(monkeypatch):
    import torch.distributed as dist
    from directvoxgo_amd.export import extract_mesh
    from directvoxgo_amd.interp import TRI_INTERP_FINE_TRAIN
    from directvoxgo_amd.train import TrainStep
    m = _model(rgbnet_dim=4)
    with pytest.raises(NotImplementedError, match='extract_mesh'):
        extract_mesh(m)
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_world_size', lambda group=None: 2)
    with pytest.raises(NotImplementedError, match='without k0'):
        TrainStep(m, TRI_INTERP_FINE_TRAIN, dict(near=0.5, far=6.0, bg=1, stepsize=0.5))


def test_optimizer_groups_follow_tri_multiscene():
    from directvoxgo_amd.interp import TRI_INTERP_FINE_TRAIN
    from directvoxgo_amd.train import create_optimizer_or_freeze_model
    m = _model(rgbnet_dim=4, interp_depth=3)
    opt = create_optimizer_or_freeze_model(m, TRI_INTERP_FINE_TRAIN, global_step=0)
    lr = {id(p): g['lr'] for g in opt.param_groups for p in g['params']}
    for net in INTERP:
        assert all(lr[id(p)] == 5e-4 for p in getattr(m, net).parameters()), net
    assert all(lr[id(p)] == 1e-3 for p in m.rgbnet.parameters())
    assert all(lr[id(p)] == TRI_INTERP_FINE_TRAIN['lrate_planes'] for p in m.planes.values())
    assert lr[id(m.density)] == TRI_INTERP_FINE_TRAIN['lrate_density'] and len(lr) == 1 + 3 + 6 + 3 * 6
    assert TRI_INTERP_FINE_TRAIN['lrate_decay'] == 1000 and TRI_INTERP_FINE_TRAIN['N_iters'] == 50000
    assert not any(k in TRI_INTERP_FINE_TRAIN for k in ('lrate_encoder', 'lrate_map', 'lrate_map_xy'))
