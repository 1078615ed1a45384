"""GPU: mesh extraction (csrc/mesh.hip, export.py) against the numpy statement (tests/mesh_oracle.py), the renderer's
field, the colour head, and the reference's volume export."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tests'))
import mesh_oracle as M  # noqa: E402

pytestmark = pytest.mark.gpu


def _model(world, rgbnet_dim=12, rgbnet_direct=False, channels_last=True, seed=777):
    from directvoxgo_amd.dvgo import DirectVoxGO
    from directvoxgo_amd.scenes import synthetic_scene
    k0_dim = rgbnet_dim if rgbnet_dim > 0 else 3
    sc = synthetic_scene(world=world, n_rays=16, seed=seed, device='cuda', k0_dim=k0_dim)
    m = DirectVoxGO(sc['xyz_min'].cpu(), sc['xyz_max'].cpu(), num_voxels=world ** 3, num_voxels_base=world ** 3,
                    alpha_init=1e-2, rgbnet_dim=rgbnet_dim, rgbnet_direct=rgbnet_direct,
                    channels_last=channels_last).cuda()
    assert tuple(m.density.shape[2:]) == (world,) * 3
    with torch.no_grad():
        m.density.copy_(sc['density']); m.k0.copy_(sc['k0']); m.mask_cache.mask.copy_(sc['mask'])
    return m


def _check_against_oracle(model, mesh_kw, alpha_thres=0.5):
    from directvoxgo_amd.export import extract_mesh, mesh_field
    field, iso, lat = mesh_field(model, alpha_thres, **mesh_kw)
    mesh = extract_mesh(model, alpha_thres, color=False, **mesh_kw)
    F = field.cpu().numpy()
    # the field the kernel built against the CPU statement of the same lattice
    mc = model.mask_cache
    ref_field = M.lattice_field(model.density.detach()[0, 0].cpu().numpy(), lat.R, lat.a, lat.s, lat.mn, lat.h, iso,
                                mask=mc.mask.cpu().numpy(), mask_scale=mc.xyz2ijk_scale.cpu().numpy(),
                                mask_shift=mc.xyz2ijk_shift.cpu().numpy(), copy=lat.copy)
    if lat.copy:
        assert np.array_equal(F, ref_field)
    else:
        np.testing.assert_allclose(F, ref_field, rtol=1e-6, atol=1e-6)
    v, f, n = M.marching_tets(F, iso, lat.mn, lat.h)
    assert len(v) > 1000
    assert mesh.vertices.shape == v.shape and mesh.faces.shape == f.shape
    ext = float(np.max(np.asarray(lat.h) * (np.array(lat.R) - 1)))
    np.testing.assert_allclose(mesh.vertices.cpu().numpy(), v, rtol=0, atol=1e-6 * ext)
    assert np.array_equal(M.canonical_faces(mesh.faces.cpu().numpy()), M.canonical_faces(f))
    np.testing.assert_allclose(mesh.normals.cpu().numpy(), n, rtol=0, atol=1e-5)
    two, once = M.half_edges_ok(f)
    assert two and once
    return mesh, F, iso, lat


def test_default_lattice_64_with_mask():
    _check_against_oracle(_model(64), {})


def test_default_lattice_160_with_mask_and_link_to_the_renderer():
    m = _model(160)
    mesh, F, iso, lat = _check_against_oracle(m, {})
    # on an x / y / z edge between two real, unmasked grid points the renderer's trilinear field is linear: it
    # equals the level at the vertex
    pts, dirs = M.vertex_edges(F, iso)
    e = M.DIRS[dirs]
    lo, hi = pts - 1, pts - 1 + e
    R = np.array(lat.R)
    mask = m.mask_cache.mask.cpu().numpy()
    sel = (dirs < 3) & (lo >= 0).all(1) & (hi < R).all(1)
    sel[sel] &= mask[tuple(lo[sel].T)] & mask[tuple(hi[sel].T)]
    assert sel.sum() > 1000
    v = mesh.vertices[torch.from_numpy(np.nonzero(sel)[0]).cuda()]
    with torch.no_grad():
        val = m.grid_sampler(v, m.density).cpu().numpy()
    np.testing.assert_allclose(val, iso, rtol=0, atol=1e-4)


def test_resampled_160_to_1_5x_through_the_trilinear_path():
    from oracle import torch_cpu
    m = _model(160)
    mesh, F, iso, lat = _check_against_oracle(m, {'resolution': 240})
    assert lat.R == (240, 240, 240) and not lat.copy
    # the lattice field against the reference's grid sampler at the unmasked points, evaluated in double at the
    # kernel's fp32 grid-index coordinates g = a + i s (an fp32 world position would move the point by ~1e-7 of the box)
    g = np.random.default_rng(1)
    ijk = g.integers(0, 240, (200000, 3))
    inner = F[1:-1, 1:-1, 1:-1][tuple(ijk.T)]
    keep = inner != np.float32(iso) - np.float32(1)
    g32 = np.float32(lat.a) + ijk.astype(np.float32) * np.float32(lat.s)
    mn, mx = m.xyz_min.cpu().double(), m.xyz_max.cpu().double()
    xyz = torch.from_numpy(mn.numpy() + g32.astype(np.float64) * ((mx - mn).numpy() / 159))
    ref = torch_cpu.grid_sampler(m.density.detach().cpu().double(), xyz, mn, mx).numpy()
    np.testing.assert_allclose(inner[keep], ref[keep], rtol=1e-5, atol=1e-5)


def test_sub_bbox():
    m = _model(160)
    _, _, _, lat = _check_against_oracle(m, {'bbox': ([-0.9, -0.5, -1.2], [0.4, 1.1, 0.3])})
    assert not lat.copy


def test_two_extractions_are_bitwise_equal():
    from directvoxgo_amd.export import extract_mesh
    m = _model(160)
    a = extract_mesh(m, 0.5)
    b = extract_mesh(m, 0.5)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    a = extract_mesh(m, 0.3, resolution=200, color=False)
    b = extract_mesh(m, 0.3, resolution=200, color=False)
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)


def test_ball_faces_wind_outward():
    from directvoxgo_amd.export import extract_mesh, iso_level
    m = _model(96, rgbnet_dim=0)
    X = 96
    I, J, K = torch.meshgrid(*[torch.arange(X, dtype=torch.float32)] * 3, indexing='ij')
    r = torch.sqrt((I - 47.3) ** 2 + (J - 46.8) ** 2 + (K - 48.1) ** 2)
    with torch.no_grad():
        m.density.copy_((iso_level(m, 0.5) + 0.5 * (30.0 - r))[None, None].cuda())
        m.mask_cache.mask.fill_(True)
    mesh = extract_mesh(m, 0.5, color=False)
    v, f, n = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy().astype(np.int64), mesh.normals.cpu().numpy()
    a, b, c = (v[f[:, k]] for k in range(3))
    fn = np.cross(b - a, c - a)
    assert ((fn * n[f].mean(1)).sum(1) > 0).all()
    assert M.euler_characteristic(len(v), f) == 2
    _, vol = M.area_and_volume(v, f)
    r0 = 30.0 * float(m.xyz_max[0] - m.xyz_min[0]) / (X - 1)
    assert abs(vol / (4 / 3 * np.pi * r0 ** 3) - 1) < 0.02


@pytest.mark.parametrize('head', ['none', 'direct', 'diffuse'])
def test_colours_are_the_colour_head_seen_from_outside(head):
    from directvoxgo_amd.export import extract_mesh
    m = _model(64, rgbnet_dim=0 if head == 'none' else 12, rgbnet_direct=head == 'direct')
    mesh = extract_mesh(m, 0.5)
    assert mesh.colors.shape == mesh.vertices.shape
    m.fused_shade = False
    with torch.no_grad():
        k0 = m.grid_sampler(mesh.vertices, m.k0)
        ref = m._shade(k0, -mesh.normals, torch.arange(mesh.vertices.shape[0], device='cuda'))[:, :3]
    np.testing.assert_allclose(mesh.colors.cpu().numpy(), ref.cpu().numpy(), rtol=1e-5, atol=1e-6)
    c = mesh.colors.cpu().numpy()
    assert c.min() >= 0 and c.max() <= 1


@pytest.mark.parametrize('channels_last', [True, False])
def test_export_volume_matches_the_activation(tmp_path, channels_last):
    from directvoxgo_amd.export import export_volume, save_volume
    from directvoxgo_amd.scenes import activate
    m = _model(64, channels_last=channels_last)
    out = export_volume(m)
    alpha = activate(m.density.detach(), m.act_shift, float(m.voxel_size_ratio))[0, 0].cpu().numpy()
    rgb = torch.sigmoid(m.k0.detach())[0].permute(1, 2, 3, 0).cpu().numpy()
    assert out['alpha'].shape == (64, 64, 64) and out['rgb'].shape == (64, 64, 64, 12)
    np.testing.assert_allclose(out['alpha'], alpha, rtol=0, atol=1e-6)
    np.testing.assert_allclose(out['rgb'], rgb, rtol=0, atol=1e-6)
    p = str(tmp_path / 'vol.npz')
    save_volume(p, m)
    z = np.load(p, allow_pickle=False)
    assert sorted(z.files) == ['alpha', 'rgb'] and z['alpha'].dtype == np.float32
    # tools/vis_volume.py takes the arrays as they are when rgb.shape[0] >= rgb.shape[-1]
    assert z['rgb'].shape[0] >= z['rgb'].shape[-1] and z['rgb'].shape[:3] == z['alpha'].shape
    assert np.array_equal(z['alpha'], out['alpha']) and np.array_equal(z['rgb'], out['rgb'])


def test_mpi_model_raises():
    from directvoxgo_amd.dmpigo import DirectMPIGO
    from directvoxgo_amd.export import extract_mesh
    m = DirectMPIGO([-1, -1, 0], [1, 1, 1], num_voxels=16 ** 3, mpi_depth=16).cuda()
    with pytest.raises(NotImplementedError):
        extract_mesh(m)
