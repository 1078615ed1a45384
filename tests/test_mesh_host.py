"""CPU: the mesh oracle (tests/mesh_oracle.py) on analytic fields, write_ply, the host side of export.py, the C-ABI
argument checks of the mesh entry points, and the wait-state lint of csrc/mesh.hip."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tests'))
import mesh_oracle as M  # noqa: E402


def _coords(n, c):
    I, J, K = np.meshgrid(*[np.arange(n, dtype=np.float64)] * 3, indexing='ij')
    return I - c[0], J - c[1], K - c[2]


def _mesh(values):
    F = M.pad_field(np.asarray(values, np.float32), 0.0)
    return M.marching_tets(F, 0.0, np.zeros(3), np.ones(3))


def _closed(faces):
    two_per_edge, once_per_half_edge = M.half_edges_ok(faces)
    assert two_per_edge and once_per_half_edge


def test_ball_is_closed_oriented_and_measures_right():
    r0 = 19.3
    x, y, z = _coords(56, (27.6, 27.2, 27.9))
    r = np.sqrt(x * x + y * y + z * z)
    v, f, nrm = _mesh(2.0 * (r0 - r))
    _closed(f)
    assert M.euler_characteristic(len(v), f) == 2
    area, vol = M.area_and_volume(v, f)
    assert abs(area / (4 * np.pi * r0 ** 2) - 1) < 0.02
    assert vol > 0 and abs(vol / (4 / 3 * np.pi * r0 ** 3) - 1) < 0.02
    # unit normals pointing outward (away from the centre)
    np.testing.assert_allclose(np.linalg.norm(nrm, axis=1), 1, rtol=1e-5)
    centre = np.array([27.6, 27.2, 27.9]) - 1          # vertex coordinates are unpadded indices here
    assert ((v - centre) * nrm).sum(1).min() > 0


def test_torus_has_euler_characteristic_zero():
    x, y, z = _coords(64, (31.5, 31.3, 31.7))
    q = np.sqrt(x * x + y * y) - 18.0
    v, f, _ = _mesh(6.5 - np.sqrt(q * q + z * z))
    _closed(f)
    assert M.euler_characteristic(len(v), f) == 0


def test_two_disjoint_balls_have_euler_characteristic_four():
    x, y, z = _coords(48, (23.5, 23.5, 23.5))
    r1 = np.sqrt((x - 11) ** 2 + y * y + z * z)
    r2 = np.sqrt((x + 11) ** 2 + y * y + z * z)
    v, f, _ = _mesh(np.maximum(9.0 - r1, 9.0 - r2))
    _closed(f)
    assert M.euler_characteristic(len(v), f) == 4


def test_empty_field_has_no_mesh():
    v, f, nrm = _mesh(-np.ones((20, 21, 22)))
    assert v.shape == (0, 3) and f.shape == (0, 3) and nrm.shape == (0, 3)


def test_all_inside_field_gives_a_closed_box():
    v, f, _ = _mesh(np.ones((9, 10, 11)))
    _closed(f)
    assert M.euler_characteristic(len(v), f) == 2
    area, vol = M.area_and_volume(v, f)
    assert vol > 9 * 10 * 11 * 0.9 and area > 0


def test_vertex_ids_follow_point_then_direction_order():
    """the numbering of DESIGN.md 6c on a hand-checkable field: one inside point in a 1x1x2 lattice"""
    F = M.pad_field(np.array([[[1.0, -1.0]]], np.float32), 0.0)
    v, f, _ = M.marching_tets(F, 0.0, np.zeros(3), np.ones(3))
    # the inside point (unpadded 0,0,0) has 14 lattice neighbours; every edge to it crosses once
    assert len(v) == 14
    _closed(f)
    assert M.euler_characteristic(len(v), f) == 2
    # vertices are listed point by point, in linear order of the edge's lower point
    lower = np.floor(v + 1e-6)
    lin = (lower[:, 0] * 3 + lower[:, 1]) * 4 + lower[:, 2]
    assert (np.diff(lin) >= 0).all()


def test_case_table_is_consistent():
    """complementary cases give the same polygon reversed, and every polygon has 3 or 4 distinct edges"""
    tab = M.case_table()
    for (t, m), poly in tab.items():
        if m in (0, 15):
            assert poly == []
            continue
        assert len(poly) == (4 if bin(m).count('1') == 2 else 3) and len(set(poly)) == len(poly)
        comp = tab[(t, 15 - m)]
        assert sorted(comp) == sorted(poly)
        k = comp.index(poly[0])
        assert comp[k::-1] + comp[:k:-1] == poly


# ---------------------------------------------------------------------------------------------- write_ply
@pytest.mark.parametrize('with_color', [True, False])
def test_write_ply_round_trip(tmp_path, with_color):
    from directvoxgo_amd.export import Mesh, write_ply
    from directvoxgo_amd.metrics import to8b
    g = np.random.default_rng(0)
    V, F = 37, 51
    v = g.standard_normal((V, 3)).astype(np.float32)
    n = g.standard_normal((V, 3)).astype(np.float32)
    c = g.uniform(-0.1, 1.1, (V, 3)).astype(np.float32)
    f = g.integers(0, V, (F, 3)).astype(np.int32)
    mesh = Mesh(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(n), torch.from_numpy(c) if with_color else None)
    path = tmp_path / 'm.ply'
    write_ply(str(path), mesh)
    raw = path.read_bytes()
    end = raw.index(b'end_header\n') + len(b'end_header\n')
    header = raw[:end].decode('ascii').splitlines()
    props = ['property float x', 'property float y', 'property float z', 'property float nx', 'property float ny',
             'property float nz']
    if with_color:
        props += ['property uchar red', 'property uchar green', 'property uchar blue']
    assert header == ['ply', 'format binary_little_endian 1.0', f'element vertex {V}', *props, f'element face {F}',
                      'property list uchar int vertex_indices', 'end_header']
    stride = 24 + (3 if with_color else 0)
    body = np.frombuffer(raw[end:end + V * stride], np.uint8).reshape(V, stride)
    xyzn = np.frombuffer(body[:, :24].tobytes(), '<f4').reshape(V, 6)
    assert np.array_equal(xyzn[:, :3], v) and np.array_equal(xyzn[:, 3:], n)
    if with_color:
        assert np.array_equal(body[:, 24:], to8b(c))
    fb = np.frombuffer(raw[end + V * stride:], np.uint8)
    assert fb.size == F * 13
    fb = fb.reshape(F, 13)
    assert (fb[:, 0] == 3).all()
    assert np.array_equal(np.frombuffer(fb[:, 1:].tobytes(), '<i4').reshape(F, 3), f)


# ---------------------------------------------------------------------------------------------- host logic
def _model(**kw):
    from directvoxgo_amd.dvgo import DirectVoxGO
    return DirectVoxGO([-1, -1, -1], [1, 1, 1], num_voxels=24 ** 3, num_voxels_base=24 ** 3, alpha_init=1e-2, **kw)


def test_iso_level_is_the_alpha_threshold():
    from directvoxgo_amd.export import iso_level
    from directvoxgo_amd.scenes import activate
    m = _model()
    for a in (0.05, 0.5, 0.9):
        iso = iso_level(m, a)
        lo, hi = activate(torch.tensor([iso - 1e-3, iso + 1e-3], dtype=torch.float64), m.act_shift,
                          float(m.voxel_size_ratio))
        assert float(lo) < a < float(hi)
    with pytest.raises(ValueError):
        iso_level(m, 1.0)


def test_lattice_default_sub_box_and_resolution():
    from directvoxgo_amd.export import lattice
    m = _model()
    X = int(m.density.shape[2])
    lat = lattice(m)
    assert lat.copy and lat.R == (X, X, X)
    lat = lattice(m, resolution=(2 * X - 1, X, 5))
    assert not lat.copy and lat.R == (2 * X - 1, X, 5)
    np.testing.assert_allclose(lat.a, 0, atol=1e-12)
    np.testing.assert_allclose(lat.s, [0.5, 1.0, (X - 1) / 4])
    lat = lattice(m, resolution=30, bbox=([-0.5, -1, 0], [0.5, 1, 0.5]))
    assert lat.R == (15, 30, 8)
    np.testing.assert_allclose(lat.mn + (np.array(lat.R) - 1) * lat.h, [0.5, 1, 0.5])
    # grid-index coordinates of the box corners
    np.testing.assert_allclose(lat.a, [0.25 * (X - 1), 0, 0.5 * (X - 1)])
    lat = lattice(m, bbox=([-0.5, -0.5, -0.5], [0.5, 0.5, 0.5]))
    np.testing.assert_allclose(lat.s, 1.0, rtol=0.05)


def test_too_large_lattice_is_rejected_before_any_allocation():
    from directvoxgo_amd.export import extract_mesh
    with pytest.raises(ValueError, match='2\\^28'):
        extract_mesh(_model(), resolution=700)


def test_mpi_scenes_have_no_mesh():
    from directvoxgo_amd.dmpigo import DirectMPIGO
    from directvoxgo_amd.export import extract_mesh
    m = DirectMPIGO([-1, -1, 0], [1, 1, 1], num_voxels=16 ** 3, mpi_depth=16)
    with pytest.raises(NotImplementedError, match='NDC'):
        extract_mesh(m)


def test_bbox_and_cams_follow_run_py():
    from directvoxgo_amd.export import export_bbox_and_cams, save_bbox_and_cams
    from directvoxgo_amd.fit import compute_bbox_by_cam_frustrm
    from directvoxgo_amd.scenes import pose_spherical
    H, W, focal = 12, 16, 20.0
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    poses = [pose_spherical(th, -30.0, 4.0).numpy() for th in (-120.0, 10.0, 75.0)]
    HW = [(H, W)] * 3
    Ks = [K] * 3
    near, far = 2.0, 6.0
    mn, mx, cams = export_bbox_and_cams(HW, Ks, poses, near, far)
    lo, hi = compute_bbox_by_cam_frustrm(HW, Ks, poses, near, far)
    assert np.array_equal(mn, lo.numpy()) and np.array_equal(mx, hi.numpy())
    assert cams.shape == (3, 5, 3)
    for c2w, cam in zip(poses, cams):
        np.testing.assert_allclose(cam[0], c2w[:3, 3], atol=1e-6)
        # corner ray [0, 0] through pixel centre (0.5, 0.5), scaled by max(near, far * 0.05) = 2
        d = np.array([(0.5 - 0.5 * W) / focal, -(0.5 - 0.5 * H) / focal, -1.0]) @ c2w[:3, :3].T
        np.testing.assert_allclose(cam[1], c2w[:3, 3] + 2.0 * d, atol=1e-5)
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, 'cams.npz')
        save_bbox_and_cams(p, HW, Ks, poses, near, far)
        z = np.load(p, allow_pickle=False)
        assert sorted(z.files) == ['cam_lst', 'xyz_max', 'xyz_min'] and z['cam_lst'].shape == (3, 5, 3)


# ---------------------------------------------------------------------------------------------- ABI and lint
@pytest.fixture(scope='module')
def lib():
    from directvoxgo_amd import build
    return ctypes.CDLL(build.build(verbose=False))


def test_mesh_entries_reject_bad_arguments_before_any_launch(lib):
    vp, i64, i, f = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
    null, one = vp(0), vp(16)
    f3 = (ctypes.c_float * 3)(0, 0, 0)
    field = lambda X, R, dens, out, copy=0: lib.dvgo_mesh_field(
        dens, i(X), i(X), i(X), null, i(0), i(0), i(0), null, null, i(R), i(R), i(R), f3, f3, f3, f3, i(copy), f(0.0),
        out, null)
    assert field(8, 8, null, one) == -1                    # null density
    assert field(8, 8, one, null) == -1                    # null output
    assert field(1, 8, one, one) == -1                     # grid too small to interpolate
    assert field(8, -3, one, one) == -1                    # negative lattice
    assert field(8, 700, one, one) == -2                   # > 2^28 padded points
    assert field(8, 9, one, one, copy=1) == -1             # a copy needs the grid's own lattice
    assert lib.dvgo_mesh_field(one, i(8), i(8), i(8), one, i(-1), i(8), i(8), null, null, i(8), i(8), i(8), f3, f3, f3, f3,
                               i(0), f(0.0), one, null) == -1   # mask with bad shape / no scale
    assert lib.dvgo_mesh_count(null, i(10), i(10), i(10), f(0.0), one, one, one, null) == -1
    assert lib.dvgo_mesh_count(one, i(10), i(-10), i(10), f(0.0), one, one, one, null) == -1
    assert lib.dvgo_mesh_count(one, i(702), i(702), i(702), f(0.0), one, one, one, null) == -2
    assert lib.dvgo_mesh_count(one, i(10), i(10), i(10), f(0.0), null, one, one, null) == -1
    emit = lambda P, nv, nf, v, n, fc: lib.dvgo_mesh_emit(one, one, one, i(P), i(P), i(P), f(0.0), f3, f3, i64(nv),
                                                          i64(nf), v, n, fc, null)
    assert emit(10, -1, 0, one, one, one) == -1
    assert emit(10, 0, -5, one, one, one) == -1
    assert emit(10, 5, 0, null, one, one) == -1
    assert emit(10, 0, 5, one, one, null) == -1
    assert emit(2, 0, 0, one, one, one) == -1
    assert emit(702, 0, 0, one, one, one) == -2
    assert emit(10, 0, 0, null, null, null) == 0           # empty mesh: nothing to launch


HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='needs hipcc')
def test_mesh_unit_passes_the_wait_state_lint(tmp_path):
    """tests/test_hazards.py holds the other units to tools/hazard_lint.py; the same check for csrc/mesh.hip."""
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    import hazard_lint as H
    from directvoxgo_amd.build import FLAGS as BUILD_FLAGS
    flags = [x for x in BUILD_FLAGS if x not in ('-shared', '-Wall', '-Wno-unused-function')] + ['-S', '--cuda-device-only']
    out = tmp_path / 'mesh.s'
    subprocess.run([HIPCC] + flags + [os.path.join(REPO, 'directvoxgo_amd', 'csrc', 'mesh.hip'), '-o', str(out)],
                   check=True, capture_output=True)
    bad, n_kernels = [], 0
    for name, items in H.parse(str(out)).items():
        if not any(k == 'ins' for k, _ in items):
            continue
        n_kernels += 1
        bad += H.check_kernel(name, items)[0]
    assert n_kernels == 5
    assert not bad, '\n'.join(bad[:20])
