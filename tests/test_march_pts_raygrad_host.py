"""Host side of the ray gradient of the marches that return positions (csrc/march_raygrad.hip; no GPU):

  boundary      include/dvgo_hip.h declares dvgo_march_ray_bwd_pts and dvgo_march_vm_ray_bwd, _lib types them, the library
                exports them, and their staged argument checks answer without a device;
  oracle        on the cases of tests/march_pts_raygrad_cases.py, records from the CPU oracle of each march: every ray has a finite
                reference; the float32 restatement of either kernel (march_pts_raygrad_oracle.evaluate32) is inside the bound;
                each planted mistake is outside it;
  models        raygrad='fused': both attributes, no get_kwargs / state-dict key, load_model; what refine_poses(fused=True)
                accepts and refuses;
  resources     the compiler's metadata of every kernel of the translation unit, march_ray_bwd_kernel's two variants
                included: no private memory, no spilled register (in the manner of tests/test_hazards_vm_xyz.py).
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import march_cases as C
import march_oracle as M
import march_pts_raygrad_cases as PC
import march_pts_raygrad_oracle as PO
import march_vm_cases as V

_F = np.float32
DENSE, VM = 'dvgo_march_ray_bwd_pts', 'dvgo_march_vm_ray_bwd'


# ------------------------------------------------------------------------------------------ boundary
@pytest.fixture(scope='module')
def lib():
    from directvoxgo_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def test_header_declares_both_entries_and_lib_types_them(lib):
    from directvoxgo_amd import _lib, build
    assert 'march_raygrad.hip' in build.SOURCES and all(h in build.HEADERS for h in ('march_records.h', 'xyz_corners.h', 'vm_common.h'))
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    decl = _lib.declarations(text)
    P, i, q, fl = _lib._Pointer, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    sig = {DENSE: [P, P, P, P, q, P, q, P, P, fl, P, P, P, fl, P, P, fl, fl, P, i, i, i, P, P, P, P, P, P],
           VM: [P, P, q, P, q, P, P, fl, P, P, P, fl, P, P, fl, fl] + [P, i, i, q, q, q] * 3 + [P, i, q, q] * 3 + [i, P, P, P, P, P, P]}
    for name in (DENSE, VM):
        assert decl[name] == (ctypes.c_int, sig[name]), name
        assert getattr(lib, name).argtypes == sig[name] and getattr(lib, name).restype is ctypes.c_int
        assert getattr(ctypes.CDLL(_lib.SO_PATH), name)                              # exported
    assert _lib.ABI_VERSION == lib.dvgo_abi_version() == 11                          # no bump
    assert 'g_p = g_p + grad_pts[3 i' in text and 'Ah = fmaf(t, dh, Ah), Aw = fmaf(t, dw, Aw), An = fmaf(u, dn, An)' in text


DENSE_NAMES = ['rec2', 'n2', 'n_steps', 'cum', 'rec_stride', 'off3', 'n_rays', 'rays_start', 'rays_dir', 'stepdist', 'xyz_min',
               'xyz_max', 'last', 'interval', 'rays_o', 'rays_d', 'near', 'far', 'density', 'X', 'Y', 'Z', 'grad_weights', 'grad_last',
               'grad_pts', 'grad_o', 'grad_d', 'stream']
DENSE_REQUIRED = ('rec2', 'n2', 'n_steps', 'off3', 'rays_start', 'rays_dir', 'xyz_min', 'xyz_max', 'last', 'rays_o', 'rays_d', 'density',
                  'grad_o', 'grad_d')


def _dense(lib, n_rays=4, stepdist=0.5, X=4, null=(), rec_stride=16, cum=False):
    """every pointer a non-null value that is never dereferenced (the calls return on validation)"""
    one = ctypes.c_void_p(16)
    vals = dict.fromkeys(DENSE_NAMES, one)
    vals.update(cum=one if cum else None, rec_stride=rec_stride, n_rays=n_rays, stepdist=stepdist, interval=0.5, near=0.0, far=1.0,
                X=X, Y=4, Z=4, stream=None)
    for k in null:
        vals[k] = None
    return lib.dvgo_march_ray_bwd_pts(*[vals[k] for k in DENSE_NAMES])


def test_dense_entry_judges_its_arguments_in_stages(lib):
    every = [k for k in DENSE_NAMES if k not in ('rec_stride', 'n_rays', 'stepdist', 'interval', 'near', 'far', 'X', 'Y', 'Z', 'stream')]
    assert _dense(lib, n_rays=-1) == -1 and _dense(lib, X=0) == -1
    assert _dense(lib, stepdist=0.0) == -1 and _dense(lib, stepdist=-255.0) == -1        # NDC spacing is not differentiated
    assert _dense(lib, n_rays=-1, null=every) == -1 and _dense(lib, stepdist=0.0, n_rays=0) == -1          # shapes first
    assert _dense(lib, n_rays=0) == 0 and _dense(lib, n_rays=0, null=every) == 0         # no pointer is looked at
    for k in DENSE_REQUIRED:
        assert _dense(lib, null=(k,)) == -1, k                                           # each required pointer is
        assert _dense(lib, n_rays=1 << 25, null=(k,)) == -1, k                           # NULL before the range
    assert _dense(lib, rec_stride=0) == -1                                               # neither layout
    assert _dense(lib, n_rays=1 << 25) == -2                                             # n_rays * 64 == 2^31
    assert _dense(lib, n_rays=1 << 25, null=('grad_last', 'grad_pts', 'grad_weights'), cum=True, rec_stride=0) == -2
    from directvoxgo_amd import _lib
    with pytest.raises(RuntimeError, match='invalid argument'):
        _lib.call(DENSE, *[None] * 4, 16, None, 4, None, None, 0.0, *[None] * 3, 0.5, None, None, 0.0, 1.0, None, 4, 4, 4, *[None] * 6)


KEYS = ('xy', 'yz', 'zx')
VM_PTRS = ('rec2', 'n2', 'off3', 'rays_start', 'rays_dir', 'xyz_min', 'xyz_max', 'last', 'rays_o', 'rays_d') + KEYS + (
    'xy_line', 'yz_line', 'zx_line', 'grad_o', 'grad_d')
VM_OPTIONAL = ('grad_weights', 'grad_last', 'grad_pts')


def _vm(lib, n_rays=4, stepdist=0.5, R=4, sizes=((6, 7), (3, 9), (8, 2)), lines=(5, 1, 9), rec_stride=16, null=()):
    one = ctypes.c_void_p(16)
    p = lambda k: None if k in null else one         # noqa: E731
    args = [p('rec2'), p('n2'), rec_stride, p('off3'), n_rays, p('rays_start'), p('rays_dir'), stepdist, p('xyz_min'), p('xyz_max'),
            p('last'), 0.5, p('rays_o'), p('rays_d'), 0.0, 1.0]
    for k, (H, W) in zip(KEYS, sizes):
        args += [p(k), H, W, 1, W * R, R]
    for k, N in zip(KEYS, lines):
        args += [p(k + '_line'), N, 1, R]
    return lib.dvgo_march_vm_ray_bwd(*args, R, p('grad_weights'), p('grad_last'), p('grad_pts'), p('grad_o'), p('grad_d'), None)


def test_vm_entry_judges_its_arguments_in_stages(lib):
    assert _vm(lib, n_rays=-1) == -1 and _vm(lib, R=0) == -1 and _vm(lib, rec_stride=0) == -1
    assert _vm(lib, stepdist=0.0) == -1 and _vm(lib, stepdist=-63.0) == -1
    assert _vm(lib, sizes=((6, 7), (0, 9), (8, 2))) == -1 and _vm(lib, lines=(5, 0, 9)) == -1
    assert _vm(lib, n_rays=0, lines=(0, 1, 9), null=VM_PTRS) == -1                       # shapes first
    assert _vm(lib, n_rays=1 << 25, sizes=((6, 7), (3, 9), (8, 0))) == -1                # ... and before the range
    assert _vm(lib, n_rays=0) == 0 and _vm(lib, n_rays=0, null=VM_PTRS + VM_OPTIONAL) == 0
    for k in VM_PTRS:
        assert _vm(lib, null=(k,)) == -1, k
        assert _vm(lib, n_rays=1 << 25, null=(k,)) == -1, k                              # NULL before the range
    assert _vm(lib, n_rays=1 << 25) == -2 and _vm(lib, rec_stride=1 << 31) == -2
    assert _vm(lib, n_rays=1 << 25, null=VM_OPTIONAL) == -2


# ------------------------------------------------------------------------------------------ oracle
def _dense_case(name, oracle):
    sc = C.fine_scene() if name == 'fine129' else PC.rand20_scene()
    return sc, C.cpu_forward(sc, oracle), dict(density=sc.density)


def _vm_case(name, oracle):
    if name.startswith('vm20'):
        sc, planes, lines = PC.vm20_scene(int(name[-1]))
    else:
        which, pad = name.split('-')
        sc = C.fine_scene() if which == 'fine129' else C.coarse_scene()
        planes, lines = V.vm_tensors(sc, pad == 'padded')
    return sc, V.cpu_forward_vm(sc, oracle, planes, lines)[0], dict(planes=planes, lines=lines)


CASES = ['fine129', 'rand20', 'fine129-padded', 'fine129-unpadded', 'coarse129-padded', 'coarse129-unpadded', 'vm20-R4', 'vm20-R5']
RANDOM = ('rand20', 'vm20-R4', 'vm20-R5')


def _setup(name, oracle):
    sc, q, model = (_dense_case if name in ('fine129', 'rand20') else _vm_case)(name, oracle)
    Rc = q.R
    o32, d32 = sc.arrays()
    N = o32.shape[0]
    t_min = oracle.sample_pts_on_rays(o32, d32, sc.xyz_min, sc.xyz_max, sc.near, sc.far, float(_F(sc.stepdist)))[5]
    dirs = (d32 / np.sqrt((d32.astype(np.float64) ** 2).sum(-1, keepdims=True))).astype(np.float32)
    off3 = np.concatenate([[0], np.cumsum(q.n3)])
    gw, gl, gp = PC.upstream(N, int(off3[-1]), 41)
    common = (Rc, q.last, M.gw_per_record(Rc, off3, gw), gl, float(_F(sc.interval)), q.start, dirs, sc.stepdist, sc.xyz_min, sc.xyz_max)
    return sc, Rc, off3, gp, common, model, t_min, d32


def _reference(common, model, gpts, t_min, d32):
    if 'density' in model:
        return PO.reference_dense(*common, model['density'], gpts, t_min, d32)
    return PO.reference_vm(*common, model['planes'], model['lines'], gpts, t_min, d32)


@pytest.mark.parametrize('name', CASES)
def test_restatement_inside_the_bound_every_ray_finite_and_each_mutant_outside(name, oracle):
    sc, Rc, off3, gp, common, model, t_min, d32 = _setup(name, oracle)
    N = Rc.n.shape[0]
    if name in RANDOM:
        assert N == 96 and Rc.ray.shape[0] > 1000 and int(off3[-1]) > 300
    elif name == 'fine129' or name.startswith('fine129'):
        assert {0, 1, 63, 64, 65, 256} <= set(Rc.n.tolist())
    assert np.any(Rc.flag)
    if sc.thres > 0:                                            # (the coarse stage has no filter: every record is kept)
        n3 = np.bincount(Rc.ray, Rc.flag, N)
        assert np.any((n3 > 0) & (n3 < Rc.n))                   # flagged and unflagged records in one ray
    rows = PO.pts_rows(Rc, off3, gp)
    for with_pts in (True, False):
        G = _reference(common, model, rows if with_pts else None, t_min, d32)
        assert G.finite.all() and np.isfinite(G.boundA).all() and np.isfinite(G.boundB).all(), np.nonzero(~G.finite)[0]
        assert float(np.abs(G.A).max()) > 1e-3 and float(np.abs(G.B).max()) > 1e-3
        go, gd = PO.evaluate32(*common, rows if with_pts else None, t_min, d32, **model)
        r = PO.check(G, go, gd, (), what=f'{name} pts={with_pts}')
        assert r <= 1.0
        print(f'\nfloat32 restatement, worst err / bound  {name} grad_pts={with_pts}: {r:.4f}', end='')
    if name not in RANDOM and name != 'fine129':
        return
    # the bound is not vacuous: every planted mistake of the float32 evaluation falls outside it
    G = _reference(common, model, rows, t_min, d32)
    everywhere = np.random.default_rng(43).standard_normal((Rc.ray.shape[0], 3)).astype(_F)
    everywhere[Rc.flag] = rows[Rc.flag]
    for mutant in PO.MUTANTS:
        go, gd = PO.evaluate32(*common, rows, t_min, d32, **model, mutant=mutant, gpts_all=everywhere)
        with pytest.raises(AssertionError, match='outside the bound'):
            PO.check(G, go, gd, (), what=f'{name} {mutant}')


# ------------------------------------------------------------------------------------------ models and pose
BASE = dict(num_voxels=10 * 12 * 14, num_voxels_base=16 ** 3, alpha_init=1e-2, fast_color_thres=1e-4)
BOX = ([-1.0, -1.2, -1.4], [1.0, 1.2, 1.4])
RK = dict(near=0.1, far=1.0, stepsize=0.5, bg=1)


def _classes():
    from directvoxgo_amd.hashgrid import HashVoxGO
    from directvoxgo_amd.tensorf import TensoRFVoxGO
    from directvoxgo_amd.vm import VMTriPlaneVoxGO
    return HashVoxGO, VMTriPlaneVoxGO, TensoRFVoxGO


def _model(cls, **kw):
    extra = {'HashVoxGO': dict(n_levels=4, n_feat=2, log2_hashmap_size=10, base_res=4, max_res=16, rgbnet_width=64),
             'VMTriPlaneVoxGO': dict(n_comp=4, rgbnet_dim=6, rgbnet_width=64),
             'TensoRFVoxGO': dict(n_comp=4, rgbnet_dim=6, rgbnet_width=64, density_n_comp=4)}[cls.__name__]
    return cls(*BOX, **{**BASE, **extra, **kw})


@pytest.mark.parametrize('which', [0, 1, 2])
def test_raygrad_fused_sets_both_attributes_and_is_no_key(which, tmp_path):
    from directvoxgo_amd.checkpoint import load_model, save_checkpoint
    cls = _classes()[which]
    m = _model(cls, raygrad='fused')
    assert m.raygrad is True and m.__dict__.get('fused_raygrad') is True and m.fused_raygrad is True
    for plain in (_model(cls), _model(cls, raygrad=True), _model(cls, raygrad=1)):
        assert 'fused_raygrad' not in plain.__dict__ and plain.fused_raygrad is False
    kw = m.get_kwargs()
    assert 'raygrad' not in kw and 'fused_raygrad' not in kw and set(kw) == set(_model(cls).get_kwargs())
    assert not any('raygrad' in k for k in m.state_dict())
    path = str(tmp_path / 'm.tar')
    save_checkpoint(path, m, None, 3)
    plain = load_model(cls, path)
    assert plain.raygrad is False and 'fused_raygrad' not in plain.__dict__
    m2 = load_model(cls, path, raygrad='fused')
    assert m2.raygrad is True and m2.__dict__.get('fused_raygrad') is True and set(m2.state_dict()) == set(m.state_dict())
    assert torch.equal(m2.density, m.density) if which < 2 else torch.equal(m2.density_planes['xy'], m.density_planes['xy'])


def _refine_args(cfg):
    from directvoxgo_amd.pose import CameraRefiner
    K = np.array([[4.0, 0, 2], [0, 4.0, 2], [0, 0, 1]], np.float32)
    ref = CameraRefiner(np.eye(4, dtype=np.float32)[None, :3], [[4, 4]], [K])
    return (ref, torch.zeros(1, 4, 4, 3), cfg, RK, 1, 8, 1e-3)


@pytest.mark.parametrize('which', [0, 1, 2])
def test_refine_poses_fused_accepts_the_model_only_with_the_option(which):
    from directvoxgo_amd.pose import refine_poses
    from directvoxgo_amd.train import FINE_TRAIN
    cls = _classes()[which]
    name = cls.__name__
    args = _refine_args(dict(FINE_TRAIN))
    march = dict(fused_march=True) if which == 2 else {}
    m = _model(cls, raygrad='fused', **march)
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):                   # accepted: the render is reached
        refine_poses(m, *args, fused=True)
    assert m.__dict__.get('fused_raygrad') is True                                     # left as it was found
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        refine_poses(m, *args)                                                         # and fused=False as before
    for plain in (_model(cls, raygrad=True, **march), _model(cls, raygrad=True, fused=False, **march)):
        with pytest.raises(ValueError, match=f"{name}.*op-by-op path only.*raygrad='fused'"):
            refine_poses(plain, *args, fused=True)
        assert 'fused_raygrad' not in plain.__dict__
    with pytest.raises(ValueError, match='needs a model on the fused march'):
        refine_poses(_model(cls, raygrad='fused', fused=False, **march), *args, fused=True)


def test_tensorf_without_fused_march_gets_the_fused_march_error():
    from directvoxgo_amd.pose import refine_poses
    from directvoxgo_amd.train import FINE_TRAIN
    cls = _classes()[2]
    m = _model(cls, raygrad='fused')
    assert m.fused_march is False
    with pytest.raises(ValueError, match='fused_march'):
        refine_poses(m, *_refine_args(dict(FINE_TRAIN)), fused=True)
    assert m.__dict__.get('fused_raygrad') is True


@pytest.mark.parametrize('which', [0, 1, 2])
def test_which_path_such_rays_take(which, monkeypatch):
    """raygrad='fused' keeps rays that require grad on the fused path where there is one, and falls back to _forward_raygrad
    silently where there is none; raygrad=True renders them op by op whatever `fused` says."""
    from directvoxgo_amd import fused as F
    from directvoxgo_amd import tensorf, triplane
    cls = _classes()[which]
    seen = []
    monkeypatch.setattr(cls, '_forward_raygrad', lambda self, *a, **k: seen.append('eager'))

    def march(*a, positions=False, raygrad=False, **k):
        seen.append(('march', positions, raygrad))
        raise StopIteration

    no_stride = []

    def march_vm(*a, raygrad=False, **k):
        seen.append(('march_vm', raygrad))
        if no_stride:
            return None
        raise StopIteration
    monkeypatch.setattr(triplane, 'fused_march', march)
    monkeypatch.setattr(tensorf, 'fused_march_vm', march_vm)
    og, d = torch.zeros(4, 3, requires_grad=True), torch.ones(4, 3)
    march_kw = dict(fused_march=True) if which == 2 else {}

    def run(m):
        seen.clear()
        try:
            m(og, d, d, **RK)
        except StopIteration:
            pass
        return list(seen)
    want = [('march_vm', True)] if which == 2 else [('march', True, True)]
    assert run(_model(cls, raygrad='fused', **march_kw)) == want
    assert run(_model(cls, raygrad='fused', fused=False, **march_kw)) == ['eager']
    assert run(_model(cls, raygrad=True, **march_kw)) == ['eager'] and run(_model(cls, raygrad=1, fused=False)) == ['eager']
    if which == 2:
        assert run(_model(cls, raygrad='fused')) == ['eager']                          # no fused_march
        no_stride.append(True)                                                         # the march answers None: no fixed stride
        assert run(_model(cls, raygrad='fused', fused_march=True)) == [('march_vm', True), 'eager']
    import inspect
    for fn in (F.fused_march, F.fused_march_vm, F.fused_march_contract):
        assert inspect.signature(fn).parameters['raygrad'].default is False


def test_default_marches_still_refuse_such_rays_before_any_launch():
    from directvoxgo_amd import _lib
    from directvoxgo_amd import fused as F
    calls = []
    orig = _lib.call
    _lib.call = lambda name, *a: calls.append(name)
    try:
        cfg = F.MarchConfig(torch.zeros(3), torch.ones(3), 0.1, 0.0, 0.5, 1e-4, 0.0, 2.0)
        og, d = torch.zeros(4, 3, requires_grad=True), torch.ones(4, 3)
        none = torch.zeros(1, 0, 4, 4, 4)
        with pytest.raises(NotImplementedError, match='positional'):
            F.fused_march(torch.zeros(1, 1, 4, 4, 4), none, og, d, cfg, positions=True)
        with pytest.raises(NotImplementedError, match='fused_march_vm.*require grad'):
            F.fused_march_vm([torch.zeros(1, 2, 4, 4)] * 3, [torch.zeros(1, 2, 4, 1)] * 3, og, d, cfg)
        ndc = F.MarchConfig(torch.zeros(3), torch.ones(3), 0.1, 0.0, 0.5, 1e-4, 0.0, 2.0, ndc_samples=8)
        with pytest.raises(NotImplementedError, match='NDC'):
            F.fused_march(torch.zeros(1, 1, 4, 4, 4), none, og, d, ndc, positions=True, raygrad=True)
        with pytest.raises(NotImplementedError, match='NDC'):
            F.fused_march_vm([torch.zeros(1, 2, 4, 4)] * 3, [torch.zeros(1, 2, 4, 1)] * 3, og, d, ndc, raygrad=True)
    finally:
        _lib.call = orig
    assert calls == []


# ------------------------------------------------------------------------------------------ resources
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='needs hipcc')
def test_kernels_of_the_unit_use_no_private_memory_and_spill_nothing(tmp_path):
    """one metadata entry per kernel: from its `.agpr_count` (the first key of an entry) to the next one's"""
    from directvoxgo_amd.build import FLAGS as BUILD_FLAGS
    flags = [f for f in BUILD_FLAGS if f not in ('-shared', '-Wall', '-Wno-unused-function')] + ['-S', '--cuda-device-only']
    out = tmp_path / 'march_raygrad.s'
    subprocess.run([HIPCC] + flags + [os.path.join(REPO, 'directvoxgo_amd', 'csrc', 'march_raygrad.hip'), '-o', str(out)],
                   check=True, capture_output=True)
    text = out.read_text()
    entries = text[text.index('amdhsa.kernels:'):].split('  - .agpr_count:')[1:]
    found = {}
    for e in entries:
        name = re.findall(r'^\s*\.symbol:\s*(\S+)\.kd\s*$', e, flags=re.M)
        assert len(name) == 1, name
        found[name[0]] = tuple(int(re.search(rf'\.{k}:\s*(\d+)', e).group(1))
                               for k in ('private_segment_fixed_size', 'vgpr_spill_count', 'sgpr_spill_count'))
    # the unit's three kernels, five with their dispatch variants (march_ray_bwd_kernel moved here from march.hip)
    assert len(found) == 5, sorted(found)
    for kernel in ('march_ray_bwd_kernel', 'march_vm_ray_bwd_kernel'):
        for vec in ('ILi4E', 'ILi1E'):
            assert sum(kernel + vec in n for n in found) == 1, (kernel, vec, sorted(found))
    assert sum('march_pts_ray_bwd_kernel' in n for n in found) == 1, sorted(found)
    assert all(v == (0, 0, 0) for v in found.values()), found
