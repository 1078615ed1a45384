"""CPU: the march over the decomposed density (csrc/march_vm.hip) without a device.

  * the edge-case table of tests/march_cases.py restated as planes and lines (tests/march_vm_cases.py) holds on the CPU
    reference alone: positions, occupancy, raw2alpha and alpha2weight from the C oracle, the density from the float64 oracle
    of the decomposition rounded to float32.  Every row of the three scenes, padded and unpadded R, none left out; n2 and
    n3 equal the dense oracle's; the record counts are the table's;
  * the two entry points: typed from the header, argument validation before any launch;
  * the host side of `fused.fused_march_vm` and of `TensoRFVoxGO(fused_march=...)`.
"""
import ctypes

import numpy as np
import pytest
import torch

import march_cases as C
import march_vm_cases as V

SCENES = V.scenes()


@pytest.fixture(scope='module')
def dense(oracle):
    """the dense CPU forward of every scene, computed once"""
    return {sc.name: C.cpu_forward(sc, oracle) for sc in SCENES}


@pytest.mark.parametrize('pad', [True, False], ids=['padded', 'unpadded'])
@pytest.mark.parametrize('sc', SCENES, ids=[s.name for s in SCENES])
def test_table_holds_on_the_restatement(sc, pad, oracle, dense):
    """The restated density differs from the trilinear one by at most one unit in the last place of the largest level in
    use below 64 (2^-18 = 3.8e-6; measured: exactly that on fine129) and not at all on the other two scenes."""
    R_pad, R_raw, n_rows, n_rec = V.TABLE[sc.name]
    planes, lines = V.vm_tensors(sc, pad)
    assert planes['xy'].shape == (1, R_pad if pad else R_raw, 9, 9) and lines['xy'].shape[2] == sc.X
    assert not any(planes[k].any() or lines[k].any() for k in ('yz', 'zx'))
    want = dense[sc.name]
    got, dens, tri = V.cpu_forward_vm(sc, oracle, planes, lines)
    worst = float(np.abs(dens.astype(np.float64) - tri.astype(np.float64)).max())
    print(sc.name, 'pad' if pad else 'raw', 'records', got.R.ray.shape[0], 'worst |vm - trilinear|', worst)
    assert worst <= (2.0 ** -18 if sc.name == 'fine129' else 0.0)
    assert len(sc.rows) == n_rows and got.R.ray.shape[0] == want.R.ray.shape[0] == n_rec
    held = [name for name, _, pred in sc.rows if pred(got)]
    assert held == [name for name, _, _ in sc.rows], set(n for n, _, _ in sc.rows) - set(held)
    assert np.array_equal(got.n2, want.n2) and np.array_equal(got.n3, want.n3) and np.array_equal(got.n_steps, want.n_steps)
    assert np.array_equal(got.R.step, want.R.step) and np.array_equal(got.R.flag, want.R.flag)
    assert int(got.n_steps.max()) < V.rec_stride(sc)


def test_record_counts_reach_the_backward_chunk_borders(dense):
    """1, 63, 64, 65, 129 records (fine129) and more than 512 (fine1025): what the GPU test of the backward kernel needs."""
    have = set(int(v) for sc in SCENES[:2] for v in dense[sc.name].n2)
    assert {1, 63, 64, 65, 129} <= have and max(have) > 512


# ---------------------------------------------------------------------------------------------- build, typing, validation
FWD, BWD = 'dvgo_march_vm_density', 'dvgo_march_vm_density_bwd'


@pytest.fixture(scope='module')
def lib():
    from directvoxgo_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def test_build_and_typing(lib):
    from directvoxgo_amd import _lib, build
    assert 'march_vm.hip' in build.SOURCES
    with open(_lib.HEADER_PATH) as f:
        decl = _lib.declarations(f.read())
    P, i, q, fl = _lib._Pointer, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    geom = [P, i, i, q, q, q] * 3 + [P, i, q, q] * 3
    assert decl[FWD] == (ctypes.c_int, [P, P, P, q, q, P, P, fl, P, i, i, i, P, P] + geom + [i, fl, fl, fl, P, P, P, P, P, P, fl, fl, P])
    assert decl[BWD] == (ctypes.c_int, [P, P, P, q, P, P, q, P, P, fl, P, fl, P, P, P, P, P])
    assert lib.dvgo_march_vm_density.argtypes == decl[FWD][1] and lib.dvgo_march_vm_density_bwd.argtypes == decl[BWD][1]
    assert _lib.ABI_VERSION == lib.dvgo_abi_version() == 11


def _fwd(lib, N=4, R=4, sizes=((6, 7), (3, 9), (8, 2)), lines=(5, 1, 9), null=(), stepdist=0.01, stride=100, mask=False,
         msize=(4, 4, 4)):
    from directvoxgo_amd._lib import f3
    one = ctypes.c_void_p(16)         # any non-null value: rejected before it could be dereferenced, or never reached
    P = lambda k: None if k in null else one         # noqa: E731
    H = lambda k: None if k in null else f3([0.0, 0.5, 1.0])         # noqa: E731  (host arrays: these are read)
    geom = []
    for k, (h, w) in zip(('xy', 'yz', 'zx'), sizes):
        geom += [P(k), h, w, 1, w * R, R]
    for k, n in zip(('xy', 'yz', 'zx'), lines):
        geom += [P(k + '_line'), n, 1, R]
    return lib.dvgo_march_vm_density(P('start'), P('dirs'), P('n_steps'), stride, N, H('mn'), H('mx'), stepdist,
                                     one if mask else None, *msize, H('scale'), H('shift'), *geom, R, 0.0, 0.5, 1e-4,
                                     P('rec2'), P('n2'), P('n3'), P('last'), P('rays_o'), P('rays_d'), 0.0, 1.0, None)


def test_forward_entry_validates_before_any_launch(lib):
    every = ('start', 'dirs', 'n_steps', 'mn', 'mx', 'xy', 'yz', 'zx', 'xy_line', 'yz_line', 'zx_line', 'rec2', 'n2', 'n3',
             'last', 'rays_o', 'rays_d')
    assert _fwd(lib, N=0) == 0 and _fwd(lib, N=0, null=every) == 0                 # a no-op that touches no pointer
    assert _fwd(lib, N=-1) == -1 and _fwd(lib, R=0) == -1 and _fwd(lib, R=-1) == -1
    for k in every:
        assert _fwd(lib, null=(k,)) == -1, k                                        # each pointer is looked at
    assert _fwd(lib, sizes=((6, 7), (0, 9), (8, 2))) == -1 and _fwd(lib, lines=(5, 0, 9)) == -1
    assert _fwd(lib, stepdist=0.0) == -1 and _fwd(lib, stepdist=-63.0) == -1      # NDC spacing is refused
    assert _fwd(lib, N=0, stepdist=-63.0) == -1 and _fwd(lib, N=0, lines=(5, 0, 9)) == -1   # ... before the no-op
    assert _fwd(lib, stride=0) == -1 and _fwd(lib, stride=-5) == -1                # only the fixed record stride
    assert _fwd(lib, mask=True, null=('scale',)) == -1 and _fwd(lib, mask=True, null=('shift',)) == -1
    assert _fwd(lib, mask=True, msize=(4, 0, 4)) == -1
    assert _fwd(lib, N=(1 << 31) // 64) == -2 and _fwd(lib, stride=1 << 31) == -2


def _bwd(lib, N=4, null=(), stepdist=0.01, stride=100):
    one = ctypes.c_void_p(16)
    P = lambda k: None if k in null else one         # noqa: E731
    return lib.dvgo_march_vm_density_bwd(P('rec2'), P('n2'), P('n_steps'), stride, P('off3'), P('off2'), N, P('start'), P('dirs'),
                                         stepdist, P('last'), 0.5, P('gw'), P('gl'), P('g_raw'), P('xyz2'), None)


def test_backward_entry_validates_before_any_launch(lib):
    need = ('rec2', 'n2', 'n_steps', 'off3', 'off2', 'start', 'dirs', 'last', 'g_raw', 'xyz2')
    assert _bwd(lib, N=0) == 0 and _bwd(lib, N=0, null=need + ('gw', 'gl')) == 0
    assert _bwd(lib, N=-1) == -1
    for k in need:
        assert _bwd(lib, null=(k,)) == -1, k
    assert _bwd(lib, stepdist=0.0) == -1 and _bwd(lib, stepdist=-63.0) == -1 and _bwd(lib, stride=0) == -1
    assert _bwd(lib, N=(1 << 31) // 64) == -2
    from directvoxgo_amd import _lib
    with pytest.raises(RuntimeError, match='invalid argument'):               # the typed call turns the code into an error
        _lib.call(BWD, None, None, None, 100, None, None, 4, None, None, 0.01, None, 0.5, None, None, None, None, None)
    with pytest.raises(TypeError, match='arguments given'):
        _lib.call(FWD, None, 1, 1)


# ---------------------------------------------------------------------------------------------- glue and model, host side
BASE = dict(num_voxels=10 * 12 * 14, num_voxels_base=16 ** 3, alpha_init=1e-2, fast_color_thres=1e-4, n_comp=4, density_n_comp=4)
BOX = ([-1.0, -1.2, -1.4], [1.0, 1.2, 1.4])
RK = dict(near=0.5, far=6.0, bg=1, stepsize=0.5)


def _model(**kw):
    from directvoxgo_amd.tensorf import TensoRFVoxGO
    return TensoRFVoxGO(*BOX, **{**BASE, **kw})


def test_get_kwargs_round_trip_and_a_checkpoint_without_the_key(tmp_path):
    from directvoxgo_amd.checkpoint import load_model, model_kwargs_of, save_checkpoint
    from directvoxgo_amd.tensorf import TensoRFVoxGO
    assert _model().fused_march is False and _model().get_kwargs()['fused_march'] is False
    m = _model(fused_march=True, density_offset=-2.0)
    kw = m.get_kwargs()
    assert m.fused_march is True and kw['fused_march'] is True
    m2 = TensoRFVoxGO(**model_kwargs_of({'model_kwargs': kw}))
    assert m2.fused_march is True and set(m2.state_dict()) == set(m.state_dict())          # no new state
    path = str(tmp_path / 'with.tar')
    save_checkpoint(path, m, None, 7)
    assert load_model(TensoRFVoxGO, path).fused_march is True
    assert load_model(TensoRFVoxGO, path, fused_march=False).fused_march is False
    old = dict(kw)
    del old['fused_march']                                       # a checkpoint written before the option existed
    m3 = TensoRFVoxGO(**model_kwargs_of({'model_kwargs': old}))
    assert m3.fused_march is False and m3.density_offset == -2.0
    assert not m.can_keep_count_on_device()
    from directvoxgo_amd.tensorf import TENSORF_FINE_TRAIN
    from directvoxgo_amd.train import TrainStep
    assert not TrainStep(m, dict(TENSORF_FINE_TRAIN), RK).can_capture()


def test_march_config_carries_the_offset_as_activate_density_forms_it():
    m = _model(fused_march=True, density_offset=-9.0)
    cfg = m._march_vm_cfg(RK['near'], RK['far'], RK['stepsize'])
    assert cfg.act_shift == float(m.act_shift + m.density_offset) and cfg.thres == 1e-4
    assert cfg.interval == float(RK['stepsize'] * m.voxel_size_ratio) and cfg.mask is m.mask_cache.mask
    assert m._march_vm_cfg(RK['near'], RK['far'], RK['stepsize']) is cfg                     # cached
    m.density_offset -= 1.0                                                                  # fit_stage's schedule
    assert m._march_vm_cfg(RK['near'], RK['far'], RK['stepsize']).act_shift == float(m.act_shift + m.density_offset)
    base = m._march_cfg(RK['near'], RK['far'], RK['stepsize'])                               # hit_coarse_geo's: untouched
    assert base.act_shift == float(m.act_shift)


def test_no_fixed_stride_is_a_fallback_not_an_error(monkeypatch):
    """`_rec_stride == 0` (an infinite far, or scratch over the budget): fused_march_vm returns None before it looks at a
    tensor, and the model's render goes on to its op-by-op path with the same arguments."""
    from directvoxgo_amd import fused as F
    m = _model(fused_march=True)
    o, d = torch.zeros(4, 3), torch.ones(4, 3)
    cfg = m._march_vm_cfg(0.5, float('inf'), 0.5)
    assert F._rec_stride(cfg, 4) == 0 and F.fused_march_vm(m.density_planes, m.density_lines, o, d, cfg) is None
    cfg = m._march_vm_cfg(0.5, 6.0, 0.5)
    assert F._rec_stride(cfg, 4) > 0
    monkeypatch.setattr(F, '_MAX_STRIDE_SCRATCH_BYTES', 0)
    assert F.fused_march_vm(m.density_planes, m.density_lines, o, d, cfg) is None
    seen = []
    monkeypatch.setattr(m, '_render_unfused', lambda *a, **k: seen.append((a, k)) or 'op by op')
    assert m.render(m.planes, o, d, d, global_step=3, **RK) == 'op by op'
    assert seen[0][0][1] is o and seen[0][0][4] == 3 and seen[0][1] == RK
    monkeypatch.undo()
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):              # a stride exists: the march is taken, and has
        m.render(m.planes, o, d, d, **RK)                                         # no CPU fallback


def test_refusals_name_the_class_or_the_function():
    from directvoxgo_amd import fused as F
    m = _model(fused_march=True)
    o, d = torch.zeros(4, 3, requires_grad=True), torch.ones(4, 3)
    with pytest.raises(NotImplementedError, match='TensoRFVoxGO'):
        m.render(m.planes, o, d, d, **RK)
    with pytest.raises(NotImplementedError, match='TensoRFVoxGO'):
        m(o.detach(), d.clone().requires_grad_(), d, **RK)
    cfg = m._march_vm_cfg(0.5, 6.0, 0.5)
    with pytest.raises(NotImplementedError, match='fused_march_vm.*require grad'):
        F.fused_march_vm(m.density_planes, m.density_lines, o, d, cfg)
    with torch.no_grad():                                                          # without grad mode the rays are constants
        with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
            F.fused_march_vm(m.density_planes, m.density_lines, o, d, cfg)
    ndc = F.MarchConfig(m.xyz_min, m.xyz_max, 1.0, 0.0, 0.5, 1e-4, 0.0, 1.0, ndc_samples=64)
    with pytest.raises(NotImplementedError, match='NDC'):
        F.fused_march_vm(m.density_planes, m.density_lines, o.detach(), d, ndc)
