"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol include/dvgo_hip.h
declares (no compute calls without a GPU).  Also: the product package never references the oracle."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def so_path():
    from directvoxgo_amd import build
    return build.build(verbose=False)


def test_library_exports_every_declared_symbol(so_path):
    hdr = open(os.path.join(REPO, 'include', 'dvgo_hip.h')).read()
    names = re.findall(r'^\s*int\s+(dvgo_\w+)\s*\(', hdr, flags=re.M)
    assert len(names) >= 24
    lib = ctypes.CDLL(so_path)
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    lib.dvgo_abi_version.restype = ctypes.c_int
    from directvoxgo_amd import _lib
    assert lib.dvgo_abi_version() == _lib.ABI_VERSION


def test_argument_validation_returns_error_codes_before_any_launch(so_path):
    """Every entry point checks sizes and pointers first and returns DVGO_EINVAL (-1) / DVGO_ERANGE (-2) without
    touching the device -- which is also what makes these calls safe on a host without a GPU."""
    lib = ctypes.CDLL(so_path)
    vp, i64, f = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    null = vp(0)
    assert lib.dvgo_raw2alpha(null, f(0), f(0.5), i64(-1), null, null, null) == -1          # negative size
    assert lib.dvgo_raw2alpha(null, f(0), f(0.5), i64(0), null, null, null) == 0            # empty input: no-op
    assert lib.dvgo_raw2alpha(null, f(0), f(0.5), i64(8), null, null, null) == -1           # null pointers
    assert lib.dvgo_exclusive_scan_i32(null, i64(4), null, null) == -1
    assert lib.dvgo_grid_grad_split(null, i64(10), ctypes.c_int(16), ctypes.c_int(12), null, null, null) == -1
    assert lib.dvgo_grid_grad_split(null, i64(0), ctypes.c_int(16), ctypes.c_int(12), null, null, null) == 0
    one = vp(16)      # any non-null value: rejected on shape before it could be dereferenced
    assert lib.dvgo_grid_grad_split(one, i64(10), ctypes.c_int(12), ctypes.c_int(12), one, one, null) == -2   # rows of 16 only
    # colour head: shapes outside the built set are DVGO_ERANGE (the caller then keeps the torch modules)
    args = [one, ctypes.c_int(12), one, ctypes.c_int(27), one, i64(5), null, one, one, one, one, one, one]
    assert lib.dvgo_shade_fwd(*args, ctypes.c_int(96), ctypes.c_int(39), ctypes.c_int(0), one, null, null, null, null, null) == -2
    assert lib.dvgo_shade_fwd(*args, ctypes.c_int(128), ctypes.c_int(38), ctypes.c_int(0), one, null, null, null, null, null) == -1  # d_in != C + E
    assert lib.dvgo_set_tuning(ctypes.c_int(99), ctypes.c_int(1)) == -1


def test_library_has_gfx950_code_object(so_path):
    out = subprocess.run(['/opt/rocm/lib/llvm/bin/llvm-readelf', '-S', so_path], capture_output=True, text=True)
    assert '.hip_fatbin' in out.stdout
    raw = open(so_path, 'rb').read()
    assert b'gfx950' in raw


def test_record_structs_are_16_bytes():
    from directvoxgo_amd import _lib
    assert ctypes.sizeof(_lib._Rec2) == 16


def test_ops_fail_loudly_without_gpu_or_library():
    """The product path has no CPU fallback: CPU tensors are rejected with the reference's error
    (lib/cuda/render_utils.cpp:40) and a missing library raises at first use."""
    import torch
    from directvoxgo_amd import _lib, render_utils
    x = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        render_utils.sample_pts_on_rays(x, x, torch.zeros(3), torch.ones(3), 0.1, 1.0, 0.1)
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        render_utils.raw2alpha(torch.zeros(4), 0.0, 0.5)
    saved, saved_path = _lib._lib, _lib.SO_PATH
    try:
        _lib._lib, _lib.SO_PATH = None, '/nonexistent/libdvgo_hip.so'
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            _lib.lib()
    finally:
        _lib._lib, _lib.SO_PATH = saved, saved_path


def test_product_package_never_touches_the_oracle():
    pkg = os.path.join(REPO, 'directvoxgo_amd')
    offenders = []
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(('.py', '.hip', '.h', '.cpp')):
                txt = open(os.path.join(root, f)).read()
                if re.search(r'^\s*(from|import)\s+oracle\b', txt, flags=re.M) or 'libdvgo_oracle' in txt \
                        or '/root/reference' in txt and f.endswith('.py') and 'import' in txt.split('/root/reference')[0][-40:]:
                    offenders.append(f)
    assert not offenders, offenders


def test_render_utils_surface_matches_reference_names():
    """the 10 callables of render_utils.cpp:144-155, positional arity included"""
    import inspect
    from directvoxgo_amd import render_utils as ru
    expect = {'infer_t_minmax': 6, 'infer_n_samples': 3, 'infer_ray_start_dir': 3, 'sample_pts_on_rays': 7,
              'sample_ndc_pts_on_rays': 5, 'maskcache_lookup': 4, 'raw2alpha': 3, 'raw2alpha_backward': 3,
              'alpha2weight': 3, 'alpha2weight_backward': 9}
    for name, n in expect.items():
        assert len(inspect.signature(getattr(ru, name)).parameters) == n, name


def _declared():
    """{name: (return type, parameter count)} read from the header independently of _lib's reader."""
    hdr = open(os.path.join(REPO, 'include', 'dvgo_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', ' ', hdr, flags=re.S)
    out = {}
    for ret, name, params in re.findall(r'^\s*(int|int64_t)\s+(dvgo_\w+)\s*\(([^)]*)\)\s*;', hdr, flags=re.M):
        out[name] = (ret, 0 if params.strip() == 'void' else params.count(',') + 1)
    return out


def test_every_declared_function_is_typed_from_the_header(so_path):
    from directvoxgo_amd import _lib
    lib, decl = _lib.lib(), _declared()
    assert len(decl) >= 60 and decl['dvgo_brick_accumulate'][1] == 38 and decl['dvgo_abi_version'][1] == 0
    for name, (ret, n) in decl.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n, name
        assert fn.restype is (ctypes.c_int64 if ret == 'int64_t' else ctypes.c_int), name
    assert sorted(n for n, (ret, _) in decl.items() if ret == 'int64_t') == [
        'dvgo_image_metrics_workspace_bytes', 'dvgo_shade_pe_record_size', 'dvgo_shade_scratch_bytes']
    assert lib.dvgo_shade_pe_record_size(128, 39) > 1 << 14 and lib.dvgo_shade_variant(-1) >= 0      # plain Python ints


def test_header_reader_rejects_what_it_does_not_recognise():
    from directvoxgo_amd import _lib
    ok = _lib.declarations('int dvgo_f(const float* a, int64_t n, void* const* t, void* stream);\nint64_t dvgo_g(void);')
    assert [len(a) for _, a in ok.values()] == [4, 0] and ok['dvgo_g'][0] is ctypes.c_int64
    assert ok['dvgo_f'][1][1] is ctypes.c_int64 and ok['dvgo_f'][1][0] is ok['dvgo_f'][1][2] is _lib._Pointer
    for bad in ('int dvgo_f(size_t n);', 'void dvgo_f(int n);', 'int dvgo_f(int);', 'int dvgo_f(float x[3]);',
                'int dvgo_f(int n); int dvgo_f(int n);', 'static int x;'):
        with pytest.raises(RuntimeError, match='cannot read'):
            _lib.declarations(bad)


def test_call_refuses_a_wrong_argument_list_before_the_device(so_path):
    """Count and width are checked on the host: too few, too many (which ctypes alone would let through) and a wrapper
    of the wrong width all raise; the argument validation of the entry points still answers through the typed functions,
    from plain Python values, tensors' stand-ins and hand-made wrappers alike."""
    from directvoxgo_amd import _lib
    vp, i64, f = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    null = vp(0)
    good = (null, f(0), f(0.5), i64(0), null, null, null)
    _lib.call('dvgo_raw2alpha', *good)
    _lib.call('dvgo_raw2alpha', None, 0.0, 0.5, 0, None, None, None)
    with pytest.raises(TypeError):
        _lib.call('dvgo_raw2alpha', *good[:-1])
    with pytest.raises(TypeError):
        _lib.call('dvgo_raw2alpha', *good, null)
    with pytest.raises(TypeError):
        _lib.call('dvgo_not_declared')
    with pytest.raises(ctypes.ArgumentError):
        _lib.call('dvgo_raw2alpha', null, f(0), f(0.5), ctypes.c_int(0), null, null, null)      # int64_t n_pts
    with pytest.raises(ctypes.ArgumentError):
        _lib.call('dvgo_raw2alpha', 'density', 0.0, 0.5, 0, None, None, None)                   # not a pointer
    with pytest.raises(RuntimeError, match='invalid argument'):
        _lib.call('dvgo_raw2alpha', None, 0.0, 0.5, -1, None, None, None)
    lib = _lib.lib()
    assert lib.dvgo_raw2alpha(null, f(0), f(0.5), i64(-1), null, null, null) == -1
    assert lib.dvgo_raw2alpha(null, f(0), f(0.5), i64(8), null, null, null) == -1
    assert lib.dvgo_exclusive_scan_i32(null, i64(4), null, null) == -1
    one = vp(16)
    assert lib.dvgo_grid_grad_split(one, i64(10), ctypes.c_int(12), ctypes.c_int(12), one, one, null) == -2
    assert lib.dvgo_grid_grad_split(one, 10, 12, 12, one, one, None) == -2
    assert lib.dvgo_set_tuning(99, 1) == -1
    import torch
    t = torch.zeros(8)                                   # a tensor converts to its address (n = 0: nothing is read)
    assert lib.dvgo_raw2alpha(t, 0.0, 0.5, 0, t, t, None) == 0
    assert _lib._Pointer.from_param(t).value == t.data_ptr() and _lib._Pointer.from_param(_lib.f3([1, 2, 3])) is not None


def test_every_literal_call_site_matches_the_header():
    """Static: each `call('dvgo_...', ...)` in the package names a declared function and, where its argument list has no
    `*`, passes the declared number of arguments.  fused.py may splat only the Adam group of `grid_step_args` (its length
    is asserted where it is splatted) and, at the two VM launches, the 30 plane-and-line arguments of `ops._vm_geom` (their
    number is asserted where the list is built, and the launch's other arguments are counted here), and neither fused.py nor masked_adam.py wraps a pointer by hand."""
    import ast
    decl, bad, sites, splats = _declared(), [], 0, []
    pkg = os.path.join(REPO, 'directvoxgo_amd')
    for fname in sorted(os.listdir(pkg)):
        if not fname.endswith('.py'):
            continue
        tree = ast.parse(open(os.path.join(pkg, fname)).read())
        for node in ast.walk(tree):
            if fname in ('fused.py', 'masked_adam.py') and isinstance(node, ast.Name) and node.id in ('ptr', '_vp'):
                bad.append((fname, node.lineno, 'hand-made pointer'))
            if not (isinstance(node, ast.Call) and getattr(node.func, 'attr', getattr(node.func, 'id', None)) == 'call'
                    and node.args and isinstance(node.args[0], ast.Constant) and str(node.args[0].value).startswith('dvgo_')):
                continue
            name, args = node.args[0].value, node.args[1:]
            sites += 1
            if name not in decl:
                bad.append((fname, node.lineno, name, 'not declared'))
            elif any(isinstance(a, ast.Starred) for a in args):
                starred = [ast.unparse(a.value) for a in args if isinstance(a, ast.Starred)]
                splats.append((fname, name, starred))
                if len(args) - 1 > decl[name][1]:
                    bad.append((fname, node.lineno, name, 'more arguments than declared'))
                if fname == 'fused.py' and starred == ['g'] and len(args) - 1 + 30 != decl[name][1]:     # ops._vm_geom's 30
                    bad.append((fname, node.lineno, name, len(args) - 1 + 30, decl[name][1]))
            elif len(args) != decl[name][1]:
                bad.append((fname, node.lineno, name, len(args), decl[name][1]))
    assert not bad, bad
    assert sites >= 50                                   # (the walk found the call sites at all)
    assert sorted(s for s in splats if s[0] == 'fused.py') == [('fused.py', 'dvgo_brick_accumulate', ['adam']),
                                                                ('fused.py', 'dvgo_march_vm_density', ['g']),
                                                                ('fused.py', 'dvgo_march_vm_ray_bwd', ['g'])]
    src = open(os.path.join(pkg, 'ops.py')).read()
    assert src.count('assert len(geom) == 30') == 1
    src = open(os.path.join(pkg, 'fused.py')).read()
    assert src.count('g, R = _vm_geom(kt)') == 2         # `g` is that list and nothing else at both launches
    assert 'assert len(adam) == len(_NO_ADAM)' in src and re.search(r'^_NO_ADAM = \((.*)\)$', src, flags=re.M).group(1).count(',') == 13
