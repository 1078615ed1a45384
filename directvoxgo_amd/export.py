"""Geometry out of a trained scene: the reference's debug exports, and a triangle mesh extracted on the device.

  export_volume / save_volume           run.py:532-553  (--export_coarse_only / --export_fine_only): alpha and
                                        sigmoid(k0) as dense volumes, an npz tools/vis_volume.py reads as it is
  export_bbox_and_cams / save_...       run.py:514-529  (--export_bbox_and_cams_only): scene box and camera frusta
  extract_mesh -> Mesh, write_ply       a closed, outward-wound surface at alpha = alpha_thres: marching tetrahedra on
                                        the Freudenthal split (csrc/mesh.hip), colours from the model's own
                                        colour head seen head-on from outside

DirectMPIGO scenes live in NDC space and have no mesh here (NotImplementedError).
"""
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib as L
from ._lib import _i64, _int, _flt, f3, ptr, stream_of
from .metrics import to8b

MAX_LATTICE_POINTS = 1 << 28        # padded lattice; vertex ids are int32 (at most 7 per point)
_BLOCK = 256                        # MESH_B of csrc/mesh.hip: points per counting workgroup
COLOR_CHUNK = 1 << 20               # vertices per colour-head call

Mesh = namedtuple('Mesh', ['vertices', 'faces', 'normals', 'colors'])
Mesh.__doc__ = """vertices [V,3] f32 world coordinates, faces [F,3] int32 (right-hand normal outward), normals [V,3] f32
(unit, towards lower density), colors [V,3] f32 in [0,1] or None.  Device tensors."""


# ------------------------------------------------------------------------------------------ reference exports
@torch.no_grad()
def export_volume(model):
    """run.py:538-539: {'alpha': activate_density(density) [X,Y,Z], 'rgb': sigmoid(k0) [X,Y,Z,C]} as float32 numpy arrays
    (any k0 layout)."""
    if getattr(model, 'density_planes', None) is not None:
        raise NotImplementedError(f'export_volume: {type(model).__name__} has neither a dense density grid nor a k0 to export')
    alpha = model.activate_density(model.density).squeeze()
    rgb = torch.sigmoid(model.k0).squeeze().permute(1, 2, 3, 0)
    return {'alpha': np.ascontiguousarray(alpha.cpu().numpy()), 'rgb': np.ascontiguousarray(rgb.cpu().numpy())}


def save_volume(path, model):
    """run.py:540: np.savez_compressed(path, alpha=..., rgb=...), the input of tools/vis_volume.py."""
    np.savez_compressed(path, **export_volume(model))


@torch.no_grad()
def export_bbox_and_cams(HW, Ks, poses, near, far, ndc=False, inverse_y=False, flip_x=False, flip_y=False):
    """run.py:516-526 for the given (training) views -> (xyz_min [3], xyz_max [3], cam_lst [n,5,3]) numpy: the box of
    fit.compute_bbox_by_cam_frustrm and per camera its centre and the far ends of its four corner rays at
    max(near, far * 0.05)."""
    from .fit import compute_bbox_by_cam_frustrm
    from .render import get_rays_of_a_view
    xyz_min, xyz_max = compute_bbox_by_cam_frustrm(HW, Ks, poses, near, far, ndc, inverse_y, flip_x, flip_y)
    cam_lst = []
    for (H, W), K, c2w in zip(HW, Ks, poses):
        c2w = torch.as_tensor(np.asarray(c2w), dtype=torch.float32)
        rays_o, rays_d, _ = get_rays_of_a_view(int(H), int(W), K, c2w, ndc, inverse_y=inverse_y, flip_x=flip_x,
                                               flip_y=flip_y)
        cam_o = rays_o[0, 0].cpu().numpy()
        cam_d = rays_d[[0, 0, -1, -1], [0, -1, 0, -1]].cpu().numpy()
        cam_lst.append(np.array([cam_o, *(cam_o + cam_d * max(near, far * 0.05))]))
    return xyz_min.cpu().numpy(), xyz_max.cpu().numpy(), np.array(cam_lst)


def save_bbox_and_cams(path, HW, Ks, poses, near, far, ndc=False, inverse_y=False, flip_x=False, flip_y=False):
    """run.py:527-529: npz with xyz_min, xyz_max, cam_lst (the --cam input of tools/vis_volume.py)."""
    xyz_min, xyz_max, cam_lst = export_bbox_and_cams(HW, Ks, poses, near, far, ndc, inverse_y, flip_x, flip_y)
    np.savez_compressed(path, xyz_min=xyz_min, xyz_max=xyz_max, cam_lst=cam_lst)


# ------------------------------------------------------------------------------------------ mesh
def iso_level(model, alpha_thres):
    """The raw density whose activated alpha (export_volume's, interval = voxel_size_ratio) is alpha_thres:
    alpha > alpha_thres <=> density > iso.  Host double."""
    a = float(alpha_thres)
    if not 0.0 < a < 1.0:
        raise ValueError(f'alpha_thres must lie in (0, 1), got {alpha_thres}')
    interval = float(model.voxel_size_ratio)
    return math.log((1.0 - a) ** (-1.0 / interval) - 1.0) - float(model.act_shift)


Lattice = namedtuple('Lattice', ['R', 'a', 's', 'mn', 'h', 'copy'])


def lattice(model, resolution=None, bbox=None):
    """The extraction lattice: R points per axis; point i has grid-index coordinates a + i s and world position
    mn + i h (host double).  Default: the density grid's own lattice (copy).  `resolution`: points on the longest axis
    of the box (int) or per axis (3 ints); `bbox`: (min [3], max [3]) sub-box, sampled at the grid's spacing unless a
    resolution is given."""
    X, Y, Z = (int(v) for v in model.density.shape[2:])
    G = np.array([X, Y, Z])
    gmn = model._xyz_min_cpu.double().numpy()
    gmx = model._xyz_max_cpu.double().numpy()
    gh = (gmx - gmn) / (G - 1)
    if resolution is None and bbox is None:
        return Lattice(tuple(G.tolist()), np.zeros(3), np.ones(3), gmn, gh, True)
    if bbox is not None:
        mn, mx = (np.asarray(v, np.float64).reshape(3) for v in bbox)
        if not (mx > mn).all():
            raise ValueError(f'bbox max {mx} must exceed its min {mn} on every axis')
    else:
        mn, mx = gmn, gmx
    ext = mx - mn
    if resolution is None:
        R = np.maximum(np.round(ext / gh).astype(np.int64) + 1, 2)
    elif np.ndim(resolution) == 0:
        R = np.maximum(np.round(int(resolution) * ext / ext.max()).astype(np.int64), 2)
    else:
        R = np.asarray(resolution, np.int64).reshape(3)
    if (R < 2).any():
        raise ValueError(f'the lattice needs at least 2 points per axis, got {R.tolist()}')
    h = ext / (R - 1)
    return Lattice(tuple(int(v) for v in R), (mn - gmn) / gh, h / gh, mn, h, False)


def _check_lattice(R):
    n = (R[0] + 2) * (R[1] + 2) * (R[2] + 2)
    if n > MAX_LATTICE_POINTS:
        raise ValueError(f'extraction lattice {R} has {n} points with its padding, more than 2^28 '
                         '(int32 vertex ids): lower the resolution or extract a sub-bbox')
    return n


@torch.no_grad()
def mesh_field(model, alpha_thres=0.5, resolution=None, bbox=None):
    """-> (padded field [Rx+2, Ry+2, Rz+2] fp32 on the density's device, iso (fp32 value), Lattice).  The field the
    extraction thresholds: density copied or sampled trilinearly, iso - 1 on the padding and where the occupancy mask
    is 0."""
    _check_model(model)
    lat = lattice(model, resolution, bbox)
    n = _check_lattice(lat.R)
    iso = float(np.float32(iso_level(model, alpha_thres)))
    density = model.density.detach()
    L.check_f32(density, 'density')
    density = density.contiguous()
    if not density.is_cuda:
        raise RuntimeError('density must be a CUDA tensor')
    X, Y, Z = (int(v) for v in density.shape[2:])
    field = torch.empty(n, dtype=torch.float32, device=density.device)
    mc = model.mask_cache
    mask, mshape, msc, msh = None, (0, 0, 0), None, None
    if mc is not None:
        mask = mc.mask.to(density.device).contiguous()
        mshape = tuple(int(v) for v in mask.shape)
        # MaskCache's own expressions on the host copies of the box (ops.MaskCache; no device read)
        ext = model._xyz_max_cpu - model._xyz_min_cpu
        scale = (torch.tensor(list(mshape), dtype=torch.float32) - 1) / ext
        msc, msh = f3(scale), f3(-model._xyz_min_cpu * scale)
    with L.device_of(density):
        L.call('dvgo_mesh_field', ptr(density), _int(X), _int(Y), _int(Z), ptr(mask), *(_int(v) for v in mshape),
               msc, msh, *(_int(v) for v in lat.R), f3(lat.a), f3(lat.s), f3(lat.mn), f3(lat.h),
               _int(1 if lat.copy else 0), _flt(iso), ptr(field), stream_of(density))
    return field.view(*(r + 2 for r in lat.R)), iso, lat


def _check_model(model):
    from .dcvgo import DirectContractedVoxGO
    from .dmpigo import DirectMPIGO
    from .dvgo import DirectVoxGO
    from .triplane import TriPlaneVoxGO
    if getattr(model, 'density_planes', None) is not None:
        raise NotImplementedError(f'extract_mesh: {type(model).__name__} has no dense density grid for the iso-surface kernels '
                                  'to read; only DirectVoxGO is supported')
    if getattr(model, 'hash_table', None) is not None:
        raise NotImplementedError(f'extract_mesh: colouring the vertices of a {type(model).__name__} (features from a hash '
                                  'table, no k0) is not built; only DirectVoxGO is supported')
    if isinstance(model, TriPlaneVoxGO):
        raise NotImplementedError('extract_mesh: colouring the vertices of a TriPlaneVoxGO (features from planes, no k0) is '
                                  'not built; only DirectVoxGO is supported')
    if isinstance(model, DirectContractedVoxGO):
        raise NotImplementedError('extract_mesh: DirectContractedVoxGO grids live in contracted space (a non-linear warp '
                                  'of the unbounded scene); only DirectVoxGO is supported')
    if isinstance(model, DirectMPIGO):
        raise NotImplementedError('extract_mesh: DirectMPIGO scenes live in NDC space (a warped frustum, not a '
                                  'world-space box); only DirectVoxGO is supported')
    if not isinstance(model, DirectVoxGO):
        raise TypeError(f'extract_mesh needs a DirectVoxGO, got {type(model).__name__}')


@torch.no_grad()
def extract_mesh(model, alpha_thres=0.5, resolution=None, bbox=None, color=True):
    """Triangle mesh of the surface alpha = alpha_thres of a DirectVoxGO -> Mesh of device tensors.

    The surface is the level set density = iso_level(model, alpha_thres) of the raw density field (inside: strictly
    above), on the lattice of `lattice(model, resolution, bbox)`, with masked-out points and a one-point border
    counted as empty: every surface is closed, also where the box cuts it.  Deterministic (no atomics).  The
    extraction reads (V, F) back once, 8 bytes, to size its outputs: that is its only host synchronisation.
    Colours: the model's colour head (_shade) at the vertices, viewed along -normal, in chunks of COLOR_CHUNK."""
    field, iso, lat = mesh_field(model, alpha_thres, resolution, bbox)
    dev = field.device
    Px, Py, Pz = (int(v) for v in field.shape)
    n = Px * Py * Pz
    W = (n + _BLOCK - 1) // _BLOCK
    edge_mask = torch.empty(n, dtype=torch.uint8, device=dev)
    partials = torch.empty(2 * W, dtype=torch.int32, device=dev)        # uint32 words
    bases = torch.empty(2 * (W + 1), dtype=torch.int32, device=dev)
    mn, h = f3(lat.mn), f3(lat.h)
    with L.device_of(field):
        st = stream_of(field)
        L.call('dvgo_mesh_count', ptr(field), _int(Px), _int(Py), _int(Pz), _flt(iso), ptr(edge_mask), ptr(partials),
               ptr(bases), st)
        V, F = (int(v) for v in bases[2 * W:].cpu().numpy().view(np.uint32))
        verts = torch.empty((V, 3), dtype=torch.float32, device=dev)
        normals = torch.empty((V, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
        L.call('dvgo_mesh_emit', ptr(field), ptr(edge_mask), ptr(bases), _int(Px), _int(Py), _int(Pz), _flt(iso), mn, h,
               _i64(V), _i64(F), ptr(verts), ptr(normals), ptr(faces), st)
    colors = vertex_colors(model, verts, normals) if color else None
    return Mesh(verts, faces, normals, colors)


@torch.no_grad()
def vertex_colors(model, verts, normals):
    """model._shade of k0 at the vertices, seen head-on from outside (view direction -normal) -> [V,3] in [0,1].
    A positional-encoding model (posbase_pe > 0) colours from the vertex positions themselves; its k0 is not read."""
    out = torch.empty((verts.shape[0], 3), dtype=torch.float32, device=verts.device)
    posenc = model.uses_posenc
    for i in range(0, verts.shape[0], COLOR_CHUNK):
        v, nrm = verts[i:i + COLOR_CHUNK], normals[i:i + COLOR_CHUNK]
        rid = torch.arange(v.shape[0], device=v.device)
        if posenc:
            rgb = model._shade_posenc(v.contiguous(), (-nrm).contiguous(), rid)
        else:
            k0 = model.grid_sampler(v, model.k0)
            rgb = model._shade(k0, (-nrm).contiguous(), rid)
        out[i:i + v.shape[0]] = rgb[:, :3]
    return out


def write_ply(path, mesh):
    """Binary little-endian PLY: vertex x y z nx ny nz (float) [red green blue (uchar, metrics.to8b)], face
    list uchar int vertex_indices."""
    v = mesh.vertices.detach().cpu().numpy().astype('<f4')
    nrm = mesh.normals.detach().cpu().numpy().astype('<f4')
    f = mesh.faces.detach().cpu().numpy().astype('<i4')
    fields = [(c, '<f4') for c in ('x', 'y', 'z', 'nx', 'ny', 'nz')]
    if mesh.colors is not None:
        fields += [(c, 'u1') for c in ('red', 'green', 'blue')]
    rec = np.empty(len(v), dtype=np.dtype(fields))
    for k, c in enumerate('xyz'):
        rec[c] = v[:, k]
        rec['n' + c] = nrm[:, k]
    if mesh.colors is not None:
        rgb = to8b(mesh.colors.detach().cpu().numpy())
        for k, c in enumerate(('red', 'green', 'blue')):
            rec[c] = rgb[:, k]
    frec = np.empty(len(f), dtype=np.dtype([('n', 'u1'), ('idx', '<i4', (3,))]))
    frec['n'] = 3
    frec['idx'] = f
    header = ['ply', 'format binary_little_endian 1.0', f'element vertex {len(v)}']
    header += [f'property float {c}' for c in ('x', 'y', 'z', 'nx', 'ny', 'nz')]
    if mesh.colors is not None:
        header += [f'property uchar {c}' for c in ('red', 'green', 'blue')]
    header += [f'element face {len(f)}', 'property list uchar int vertex_indices', 'end_header']
    with open(path, 'wb') as fh:
        fh.write(('\n'.join(header) + '\n').encode('ascii'))
        fh.write(rec.tobytes())
        fh.write(frec.tobytes())
