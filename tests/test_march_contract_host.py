"""CPU: the fused march over contracted space (csrc/march_contract.hip) without a device.

  * every case of tests/march_contract_cases.py hits the edge it is in the table for, on the numpy restatement alone;
  * the three entry points: in the header and the library, typed from the header, argument validation before any launch;
  * the host side of `fused.fused_march_contract` and of `DirectContractedVoxGO(fused_march=...)`.
"""
import ctypes

import numpy as np
import pytest
import torch

import march_contract_cases as K

CASES = K.cases()


@pytest.fixture(scope='module')
def restated(oracle):
    return {c.name: K.cpu_forward(c) for c in CASES}


@pytest.mark.parametrize('c', CASES, ids=[c.name for c in CASES])
def test_table_hits_its_edges_on_the_restatement(c, restated):
    f = restated[c.name]
    assert c.n_max == K.TABLE[c.name][4] == c.t_tab.shape[0] and c.rays_o.shape == (c.N, 3)
    assert np.abs(c.density).max() <= 20 and np.isfinite(f['alpha']).all() and np.isfinite(f['last']).all()
    stop = f['stop_step']
    if c.name in ('partial42', 'empty'):
        assert c.n_max < 64                                           # one partial chunk
    if c.name == 'b05_l2':
        assert c.n_max == 66                                          # a second chunk of two lanes
    if c.name == 'three162':
        assert 128 < c.n_max <= 192
    if c.scene == 'wall':
        assert (stop >= 0).all() and (stop < 64).all() and (f['n2'] >= 1).all()
    if c.name in ('three162', 'b05_fog'):
        assert (stop >= 64).any()                                     # a stop in a later chunk
    if c.scene == 'empty':
        assert f['n_cand'].sum() > 0 and not f['n2'].any()            # candidates exist; the alpha filter drops them all
    if c.mask_kind == 'false':
        assert f['n_cand'].sum() == 0
    if c.mask_kind == 'half':
        full = np.bincount(K.U.sample(c.rays_o, c.rays_d, c.center, c.radius, c.world, c.stepsize, c.b, c.norm)[1], minlength=c.N)
        assert (f['n_cand'] < full).any() and f['n_cand'].sum() > 0   # the half-space cuts some rays and not everything
    if c.name == 'carry82':
        assert (f['step'] == 63).any() and (f['step'] == 64).any() and (f['step'] > 64).any()
    if c.name == 'lengths':
        assert tuple(f['n2']) == K.LENGTHS
    if c.thres == 0:
        assert np.array_equal(f['n2'], f['n3'])


def test_table_covers_the_parameters():
    rows = list(K.TABLE.values())
    assert {(r[3], r[2]) for r in rows} >= {('inf', 0.2), ('inf', 0.5), ('l2', 0.2), ('l2', 0.5)}
    assert {r[5] for r in rows} >= {1, 7, 65} and {r[8] for r in rows} == {0.0, 1e-4}
    assert {r[7] for r in rows} >= {'none', 'true', 'false', 'half'} and {r[6] for r in rows} >= {'empty', 'wall', 'fog'}
    o, d = K.special_rays()
    n = np.abs(o).max(-1)
    assert n[0] < 1 and n[1] > 1 and n[4] == 1.0 and abs(d[3][0]) == abs(d[3][1])           # inside, shell, graze, tie


# ---------------------------------------------------------------------------------------------- build, typing, validation
FWD, BWD, POS = 'dvgo_march_contract_density', 'dvgo_march_contract_density_bwd', 'dvgo_contract_positions'


@pytest.fixture(scope='module')
def lib():
    from directvoxgo_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def test_build_and_typing(lib):
    from directvoxgo_amd import _lib, build
    assert 'march_contract.hip' in build.SOURCES and 'contract_common.h' in build.HEADERS and 'march_records.h' in build.HEADERS
    with open(_lib.HEADER_PATH) as f:
        decl = _lib.declarations(f.read())
    P, i, q, fl = _lib._Pointer, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    head = [P, P, q, P, P, P, i, fl, i]
    assert decl[FWD] == (ctypes.c_int, head + [fl, P, i, i, i, P, P, P, i, i, i, P, P, fl, fl, fl, q, P, P, P, P, P])
    assert decl[BWD] == (ctypes.c_int, [P, P, q, P, P, q, P, P, P, P, P, i, fl, i, P, fl, P, P, P, P, P])
    assert decl[POS] == (ctypes.c_int, head + [P, P, q, P, P, P])
    for name in (FWD, BWD, POS):
        assert getattr(lib, name).argtypes == decl[name][1]
    assert _lib.ABI_VERSION == lib.dvgo_abi_version()


def _host3():
    from directvoxgo_amd._lib import f3
    return f3([0.0, 0.5, 1.0])


ONE = ctypes.c_void_p(16)         # any non-null value: rejected before it could be dereferenced, or never reached


def _fwd(lib, N=4, n_max=42, stride=42, null=(), mask=False, msize=(4, 4, 4), dims=(8, 8, 8)):
    P = lambda k: None if k in null else ONE         # noqa: E731
    H = lambda k: None if k in null else _host3()    # noqa: E731  (host arrays: these are read)
    return lib.dvgo_march_contract_density(P('rays_o'), P('rays_d'), N, H('center'), H('radius'), P('t_tab'), n_max, 0.2, 0, 0.05,
                                           ONE if mask else None, *msize, H('scale'), H('shift'), P('density'), *dims, H('mn'),
                                           H('mx'), 0.0, 0.5, 1e-4, stride, P('rec2'), P('n2'), P('n3'), P('last'), None)


def test_forward_entry_validates_before_any_launch(lib):
    every = ('rays_o', 'rays_d', 'center', 'radius', 't_tab', 'density', 'mn', 'mx', 'rec2', 'n2', 'n3', 'last')
    assert _fwd(lib, N=0) == 0 and _fwd(lib, N=0, null=every) == 0                 # a no-op that touches no pointer
    assert _fwd(lib, N=-1) == -1
    for k in every:
        assert _fwd(lib, null=(k,)) == -1, k                                        # each pointer is looked at
    assert _fwd(lib, n_max=0, stride=1) == -1 and _fwd(lib, n_max=-3, stride=1) == -1 and _fwd(lib, N=0, n_max=0) == -1
    assert _fwd(lib, stride=41) == -1 and _fwd(lib, stride=0) == -1 and _fwd(lib, N=0, stride=41) == -1
    assert _fwd(lib, dims=(8, 0, 8)) == -1 and _fwd(lib, dims=(-1, 8, 8)) == -1
    assert _fwd(lib, mask=True, null=('scale',)) == -1 and _fwd(lib, mask=True, null=('shift',)) == -1
    assert _fwd(lib, mask=True, msize=(4, 0, 4)) == -1
    assert _fwd(lib, N=(1 << 31) // 64) == -2 and _fwd(lib, stride=1 << 31) == -2 and _fwd(lib, dims=(2048, 2048, 2048)) == -2


def _bwd(lib, N=4, n_max=42, stride=42, null=()):
    P = lambda k: None if k in null else ONE         # noqa: E731
    H = lambda k: None if k in null else _host3()    # noqa: E731
    return lib.dvgo_march_contract_density_bwd(P('rec2'), P('n2'), stride, P('off3'), P('off2'), N, P('rays_o'), P('rays_d'),
                                               H('center'), H('radius'), P('t_tab'), n_max, 0.2, 1, P('last'), 0.5, P('gw'),
                                               P('gl'), P('g_raw'), P('q2'), None)


def test_backward_entry_validates_before_any_launch(lib):
    need = ('rec2', 'n2', 'off3', 'off2', 'rays_o', 'rays_d', 'center', 'radius', 't_tab', 'last', 'g_raw', 'q2')
    assert _bwd(lib, N=0) == 0 and _bwd(lib, N=0, null=need + ('gw', 'gl')) == 0
    assert _bwd(lib, N=-1) == -1 and _bwd(lib, n_max=0, stride=1) == -1 and _bwd(lib, stride=41) == -1
    for k in need:
        assert _bwd(lib, null=(k,)) == -1, k
    assert _bwd(lib, N=(1 << 31) // 64) == -2 and _bwd(lib, stride=1 << 31) == -2
    from directvoxgo_amd import _lib
    with pytest.raises(RuntimeError, match='invalid argument'):               # the typed call turns the code into an error
        _lib.call(BWD, None, None, 42, None, None, 4, None, None, None, None, None, 42, 0.2, 0, None, 0.5, None, None, None, None, None)
    with pytest.raises(TypeError, match='arguments given'):
        _lib.call(FWD, None, 1, 1)


def _pos(lib, N=4, M=10, n_max=42, null=()):
    P = lambda k: None if k in null else ONE         # noqa: E731
    H = lambda k: None if k in null else _host3()    # noqa: E731
    return lib.dvgo_contract_positions(P('rays_o'), P('rays_d'), N, H('center'), H('radius'), P('t_tab'), n_max, 0.2, 0, P('ray_id'),
                                       P('step_id'), M, P('q'), P('t'), None)


def test_positions_entry_validates_before_any_launch(lib):
    need = ('rays_o', 'rays_d', 'center', 'radius', 't_tab', 'ray_id', 'step_id', 'q', 't')
    assert _pos(lib, M=0) == 0 and _pos(lib, M=0, null=need) == 0
    assert _pos(lib, M=-1) == -1 and _pos(lib, N=-1) == -1 and _pos(lib, n_max=0) == -1
    for k in need:
        assert _pos(lib, null=(k,)) == -1, k
    assert _pos(lib, M=1 << 31) == -2 and _pos(lib, N=1 << 31) == -2


# ---------------------------------------------------------------------------------------------- glue and model, host side
def _model(**kw):
    from directvoxgo_amd.dcvgo import DirectContractedVoxGO
    args = dict(xyz_min=[-1, -2, -0.5], xyz_max=[1, 2, 1.5], num_voxels=24 ** 3, num_voxels_base=24 ** 3, alpha_init=1e-2, bg_len=0.2,
                fast_color_thres=1e-4)
    args.update(kw)
    return DirectContractedVoxGO(**args)


RK = dict(near=0.0, far=1e4, bg=1, stepsize=0.5)


def test_option_is_a_plain_attribute_and_survives_load_model(tmp_path):
    """tests/test_host_logic.py pins the exact key set of get_kwargs for this class, so the option is a constructor argument and
    a plain attribute (as DirectVoxGO.fused_raygrad is): a checkpoint carries no trace of it, `load_model` takes it as an
    override, and a checkpoint written before the option existed loads as it always did."""
    from directvoxgo_amd.checkpoint import load_model, model_kwargs_of, save_checkpoint
    from directvoxgo_amd.dcvgo import DirectContractedVoxGO
    assert _model().fused_march is False and _model(fused_march=True).fused_march is True and _model(fused_march=1).fused_march is True
    m = _model(fused_march=True, contracted_norm='l2')
    kw = m.get_kwargs()
    assert 'fused_march' not in kw and set(kw) == set(_model().get_kwargs()) and not any('fused_march' in k for k in m.state_dict())
    assert DirectContractedVoxGO(**model_kwargs_of({'model_kwargs': kw})).fused_march is False
    path = str(tmp_path / 'c.tar')
    save_checkpoint(path, m, None, 3)
    assert load_model(DirectContractedVoxGO, path).fused_march is False
    m2 = load_model(DirectContractedVoxGO, path, fused_march=True)
    assert m2.fused_march is True and m2.contracted_norm == 'l2' and set(m2.state_dict()) == set(m.state_dict())
    from directvoxgo_amd.train import COARSE_TRAIN, TrainStep
    assert not TrainStep(m, dict(COARSE_TRAIN), RK).can_capture() and not m.can_keep_count_on_device()


def test_march_config_restates_the_model():
    from directvoxgo_amd import dcvgo
    m = _model(fused_march=True, contracted_norm='l2', bg_len=0.5)
    cfg = m._march_contract_cfg(0.5, 'cpu')
    t, _, n_max = dcvgo.contracted_t_table(m.world, 0.5, 0.5)
    assert cfg.n_max == n_max and np.array_equal(cfg.t_tab.numpy(), t) and cfg.l2 == 1 and cfg.bg_len == 0.5
    assert cfg.thin_thres == dcvgo.thinning_threshold(m.world, 0.5, 0.5) and cfg.thres == 1e-4
    assert cfg.act_shift == float(m.act_shift) and cfg.interval == float(0.5 * m.voxel_size_ratio)
    assert list(cfg.center_h) == m.scene_center.tolist() and list(cfg.radius_h) == m.scene_radius.tolist()
    assert list(cfg.xyz_min_h) == m.xyz_min.tolist() == [-1.5] * 3 and list(cfg.xyz_max_h) == [1.5] * 3
    assert cfg.mask is m.mask_cache.mask and list(cfg.scale_h) == m.mask_cache.xyz2ijk_scale.tolist()
    assert m._march_contract_cfg(0.5, 'cpu') is cfg and m._march_contract_cfg(1.0, 'cpu') is not cfg         # cached per step size
    m._set_mask_cache(torch.zeros(tuple(m.mask_cache.mask.shape), dtype=torch.bool))                         # a new mask: a new config
    cfg2 = m._march_contract_cfg(0.5, 'cpu')
    assert cfg2 is not cfg and cfg2.mask is m.mask_cache.mask and not bool(cfg2.mask.any())
    from directvoxgo_amd.fused import ContractMarchConfig
    with pytest.raises(ValueError, match='contracted_norm'):
        ContractMarchConfig(m.scene_center, m.scene_radius, cfg.t_tab, 0.5, 'l1', 0.1, m.xyz_min, m.xyz_max, 0.0, 0.5, 0.0)


def test_fallback_above_the_scratch_budget_and_refusals(monkeypatch):
    from directvoxgo_amd import fused as F
    m = _model(fused_march=True)
    o, d = torch.zeros(4, 3), torch.ones(4, 3)
    cfg = m._march_contract_cfg(0.5, 'cpu')
    monkeypatch.setattr(F, '_MAX_STRIDE_SCRATCH_BYTES', cfg.n_max * 4 * 16 - 1)
    assert F.fused_march_contract(m.density, o, d, cfg) is None                     # before it looks at a tensor
    seen = []
    monkeypatch.setattr(m, 'sample_ray', lambda *a, **k: seen.append(a) or (_ for _ in ()).throw(KeyError('op by op')))
    with pytest.raises(KeyError, match='op by op'):                                 # the model goes on to its op-by-op path
        m(o, d, d, **RK)
    assert seen and seen[0][0] is o
    monkeypatch.undo()
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):                # the budget allows it: the march is taken, and
        m(o, d, d, **RK)                                                            # has no CPU fallback
    og = torch.zeros(4, 3, requires_grad=True)
    with pytest.raises(NotImplementedError, match='DirectContractedVoxGO'):
        m(og, d, d, **RK)
    with pytest.raises(NotImplementedError, match='DirectContractedVoxGO'):
        m(o, d.clone().requires_grad_(), d, **RK)
    with pytest.raises(NotImplementedError, match='fused_march_contract.*require grad'):
        F.fused_march_contract(m.density, og, d, cfg)
    with torch.no_grad():                                                           # without grad mode the rays are constants
        with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
            F.fused_march_contract(m.density, og, d, cfg)
    assert not _model().fused_march                                                 # and the default never reaches the march
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        _model()(o, d, d, **RK)
