"""CPU: the order in which the eight entry points that take three planes judge their arguments (csrc/plane2d.h: tp_check),
without a device: `run` (and VM's `mode`), then shapes -> -1, then M == 0 or C == 0 -> 0 with no pointer looked at, then
NULL pointers -> -1, then the 32-bit launch range -> -2.  Each case sets off two stages at once and names the one that
answers."""
import ctypes

import pytest

FWD = ('dvgo_triplane_fwd', 'dvgo_liif_gather', 'dvgo_plane_rows_fwd', 'dvgo_vm_fwd')
BWD = ('dvgo_triplane_bwd', 'dvgo_liif_scatter', 'dvgo_plane_rows_bwd', 'dvgo_vm_bwd')
KEYS = ('xy', 'yz', 'zx')
SIZES = ((6, 7), (3, 9), (8, 2))
POINTERS = KEYS + ('xy_line', 'yz_line', 'zx_line', 'xyz', 'mn', 'mx', 'io', 'io2')
GRADS = ('g_xy', 'g_yz', 'g_zx', 'gl_xy', 'gl_yz', 'gl_zx')
BIG = (1 << 31) // 12 + 1             # M * 3C >= 2^31 at C = 4, and every other entry's product is larger


@pytest.fixture(scope='module')
def lib():
    from directvoxgo_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def _call(lib, name, M=8, C=4, sizes=SIZES, lines=(5, 1, 9), ws=(5, 6, 7), P=2, null=(), run=0, mode=0):
    one = ctypes.c_void_p(16)         # any non-null value: rejected before it could be dereferenced, or never reached
    p = lambda k: None if k in null else one         # noqa: E731
    planes = []
    for k, (H, W) in zip(KEYS, sizes):
        planes += [p(k), H, W, 1, W * C, C]
    if 'vm' in name:
        for k, N in zip(KEYS, lines):
            planes += [p(k + '_line'), N, 1, C]
    tail = [C, p('xyz'), p('mn'), p('mx'), M]
    fn = getattr(lib, name)
    if name == 'dvgo_triplane_fwd':
        return fn(*planes, *tail, 0, p('io'), None)
    if name == 'dvgo_triplane_bwd':
        return fn(p('io'), *planes, *tail, 0, run, None)
    if name == 'dvgo_liif_gather':
        return fn(*planes, *tail, *ws, 1, 1, p('io'), p('io2'), None)
    if name == 'dvgo_liif_scatter':
        return fn(p('io'), *planes, *tail, *ws, 1, 1, run, None)
    if name == 'dvgo_plane_rows_fwd':
        return fn(*planes, *tail, *ws, P, 1, p('io'), None)
    if name == 'dvgo_plane_rows_bwd':
        return fn(p('io'), *planes, *tail, *ws, P, 1, run, None)
    if name == 'dvgo_vm_fwd':
        return fn(*planes, *tail, p('io'), None)
    assert name == 'dvgo_vm_bwd'
    return fn(p('io'), *planes, *[p(k) for k in GRADS], *tail, run, mode, None)


@pytest.mark.parametrize('name', FWD + BWD)
def test_stage_order(lib, name):
    assert _call(lib, name, M=BIG) == -2                                             # the range alone
    assert _call(lib, name, M=BIG, sizes=((6, 7), (0, 9), (8, 2))) == -1             # shapes before the range
    assert _call(lib, name, M=BIG, sizes=((6, 7), (3, 9), (8, 0))) == -1
    assert _call(lib, name, M=BIG, null=('xyz',)) == -1                              # NULL before the range
    assert _call(lib, name, M=BIG, C=0, null=POINTERS + GRADS) == 0                  # nothing to do before NULL and the range
    assert _call(lib, name, M=0, null=POINTERS + GRADS) == 0


@pytest.mark.parametrize('name', BWD)
def test_run_is_judged_first(lib, name):
    assert _call(lib, name, M=0, run=-1) == -1
    assert _call(lib, name, M=0, run=-1, null=POINTERS + GRADS) == -1


@pytest.mark.parametrize('name', ['dvgo_liif_gather', 'dvgo_liif_scatter', 'dvgo_plane_rows_fwd', 'dvgo_plane_rows_bwd'])
def test_world_extents_are_shapes(lib, name):
    assert _call(lib, name, M=0, ws=(0, 6, 7)) == -1
    if 'plane_rows' in name:
        assert _call(lib, name, M=0, P=0) == -1


@pytest.mark.parametrize('name', ['dvgo_vm_fwd', 'dvgo_vm_bwd'])
def test_line_lengths_are_shapes(lib, name):
    assert _call(lib, name, M=0, lines=(5, 0, 9)) == -1
    assert _call(lib, name, M=BIG, lines=(0, 1, 9)) == -1


def test_vm_bwd_looks_at_its_gradient_pointers_last(lib):
    name = 'dvgo_vm_bwd'
    for k in GRADS:
        assert _call(lib, name, M=0, null=(k,)) == 0, k
        assert _call(lib, name, M=BIG, null=(k,)) == -2, k                           # behind the range
        assert _call(lib, name, null=(k,)) == -1, k
    assert _call(lib, name, M=0, mode=3) == -1                                       # mode with run, ahead of everything
