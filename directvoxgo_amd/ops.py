"""Autograd ops and small modules of the hot path, host side.

Mirrors the Python operator surface of the reference (same names, argument meaning and
saved-tensor conventions) on top of the HIP kernels:

  Raw2Alpha, Alphas2Weights   lib/dvgo.py:618-660
  MaskCache                   lib/dvgo.py:583-613
  grid_sample                 lib/dvgo.py:312-328 (grid_sampler -> F.grid_sample + its backward, w.r.t. the grid and the positions)
  ray_points                  sample positions as a function of their rays (no counterpart: the reference's poses are constants)
  contract_points             contracted sample positions as a function of their rays (no counterpart; csrc/contract_raygrad.hip)
  triplane_sample             lib/tri_dvgo.py:456-469 (grid_sampler2D -> three F.grid_sample, cat or sum, + backward)
  liif_gather, liif_blend,    lib/tri_dvgo.py:481-565 (liif_interpolate: nearest-texel rows, blend weights, blend, + backward;
  liif_decode                 the Interp_MLPs between them stay torch modules)
  plane_rows, interp_decode   lib/tri_dvgo.py:568-607 (interpolate, liif=False: bilinear features, sampled coordinates and their
                              encoding as one MLP input row per plane, + backward; the Interp_MLPs stay torch modules)
  vm_sample                   TensoRF's vector-matrix features (no counterpart in the reference): per component a plane's
                              bilinear value times a line's linear value, + backward into planes and lines and, with
                              position_grad=True, into the positions (csrc/vm_xyz.hip)
  vm_density                  TensoRF's vector-matrix density (no counterpart in the reference): the same 3R products summed
                              on chip into one float per sample, + backward from one float of gradient per sample
                              (position_grad=True: into the positions as well, csrc/vm_xyz.hip)
  hash_sample                 Instant-NGP's multiresolution hash-grid features (no counterpart in the reference): L trilinear
                              levels, dense or hashed, in one table, + backward into the table and, with
                              position_grad=True, into the positions (csrc/hash_xyz.hip)
  segment_coo                 torch_scatter.segment_coo(src, index, out, reduce='sum')
  total_variation_add_grad    lib/cuda/total_variation.cpp:16-24
  plane_reg_add_grad          total variation and L1 of the tri-plane models' planes and lines added to their gradients, one
                              launch for all of them (no counterpart in the reference)
"""
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from . import render_utils as render_utils_hip
from ._lib import check_f32, check_input, stream_of


class Raw2Alpha(torch.autograd.Function):
    """alpha = 1 - (1 + exp(density + shift)) ** (-interval)   (lib/dvgo.py:618-642)"""

    @staticmethod
    def forward(ctx, density, shift, interval):
        exp, alpha = render_utils_hip.raw2alpha(density, shift, interval)
        if density.requires_grad:
            ctx.save_for_backward(exp)
            ctx.interval = interval
        return alpha

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_back):
        exp = ctx.saved_tensors[0]
        return render_utils_hip.raw2alpha_backward(exp, grad_back.contiguous(), ctx.interval), None, None


class Alphas2Weights(torch.autograd.Function):
    """weights_i = T_i * alpha_i with early stop, plus the residual transmittance
    (lib/dvgo.py:644-660)."""

    @staticmethod
    def forward(ctx, alpha, ray_id, N):
        weights, T, alphainv_last, i_start, i_end = render_utils_hip.alpha2weight(alpha, ray_id, N)
        if alpha.requires_grad:
            ctx.save_for_backward(alpha, weights, T, alphainv_last, i_start, i_end)
            ctx.n_rays = N
        return weights, alphainv_last

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_weights, grad_last):
        alpha, weights, T, alphainv_last, i_start, i_end = ctx.saved_tensors
        grad = render_utils_hip.alpha2weight_backward(
            alpha, weights, T, alphainv_last, i_start, i_end, ctx.n_rays,
            grad_weights.contiguous(), grad_last.contiguous())
        return grad, None, None


def _grid_geom(grid):
    """grid [1,C,X,Y,Z] (any dense strides) -> (C,X,Y,Z, sC,sX,sY,sZ) in elements."""
    if grid.dim() != 5 or grid.shape[0] != 1:
        raise RuntimeError('grid must be [1,C,X,Y,Z]')
    _, C, X, Y, Z = grid.shape
    _, sC, sX, sY, sZ = grid.stride()
    return C, X, Y, Z, sC, sX, sY, sZ


class _GridSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grid, xyz, xyz_min, xyz_max):
        if not grid.is_cuda:
            raise RuntimeError('grid must be a CUDA tensor')
        check_f32(grid, 'grid')
        check_input(xyz, 'xyz'); check_f32(xyz, 'xyz')
        C, X, Y, Z, sC, sX, sY, sZ = _grid_geom(grid)
        M = xyz.shape[0]
        out = torch.empty((M, C), dtype=torch.float32, device=xyz.device)
        with L.device_of(xyz):
            L.call('dvgo_grid_sample_fwd', grid, C, X, Y, Z, sC, sX, sY, sZ, xyz, xyz_min, xyz_max, M, out, stream_of(xyz))
        if ctx.needs_input_grad[1]:       # the position gradient reads the grid's values, not only its geometry
            ctx.save_for_backward(xyz, xyz_min, xyz_max, grid)
        else:
            ctx.save_for_backward(xyz, xyz_min, xyz_max)
        ctx.geom = (C, X, Y, Z, sC, sX, sY, sZ)
        ctx.grid_meta = grid
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        xyz, xyz_min, xyz_max = ctx.saved_tensors[:3]
        grad_grid = grad_xyz = None
        if ctx.needs_input_grad[1]:
            grid = ctx.saved_tensors[3]
            grad_out = grad_out.contiguous()
            grad_xyz = torch.empty_like(xyz)                 # every row is written by the kernel
            with L.device_of(xyz):
                L.call('dvgo_grid_sample_bwd_xyz', grid, *ctx.geom, grad_out, xyz, xyz_min, xyz_max, xyz.shape[0], grad_xyz,
                       stream_of(xyz))
        if ctx.needs_input_grad[0]:
            grad_out = grad_out.contiguous()
            # zero-filled, same strides as the parameter (F.grid_sample's backward does the same)
            grad_grid = torch.zeros_like(ctx.grid_meta, memory_format=torch.preserve_format)
            assert grad_grid.stride() == ctx.grid_meta.stride()
            with L.device_of(xyz):
                L.call('dvgo_grid_sample_bwd', grad_out, *ctx.geom, xyz, xyz_min, xyz_max, xyz.shape[0], grad_grid,
                       stream_of(xyz))
        return grad_grid, grad_xyz, None, None


def grid_sample(grid, xyz, xyz_min, xyz_max):
    """Trilinear interpolation with the exact contract of DirectVoxGO.grid_sampler
    (lib/dvgo.py:312-328): xyz [...,3] world coordinates -> [...,C], squeezed when C == 1.
    Differentiable w.r.t. ``grid`` and, when it requires grad, w.r.t. ``xyz`` (csrc/grid_sample_xyz.hip: the derivative of
    the cell the forward chose, zero padding outside the grid; once differentiable)."""
    shape = xyz.shape[:-1]
    flat = xyz.reshape(-1, 3).contiguous()
    out = _GridSample.apply(grid, flat, xyz_min.contiguous(), xyz_max.contiguous())
    out = out.reshape(*shape, grid.shape[1])
    if out.shape[-1] == 1:
        out = out.squeeze(-1)
    return out


PLANE_KEYS = ('xy', 'yz', 'zx')
# Planes that are not channels-last are handed to the kernels as channels-last copies (and their gradients scattered
# into channels-last buffers) once the samples outnumber the largest plane's texels: the copies are three passes over a
# few MB, and the kernels' 16-byte texel loads and contiguous atomic runs need that layout.  Below it the kernels run on
# the strides as given (they take either layout).  False keeps them on the given strides at every size
# (tests/test_gpu_plane_ops.py runs the strided branch that way).
TRIPLANE_RELAYOUT = True


def _plane_geom(plane, name):
    """plane [1,C,H,W] (any dense strides) -> (H, W, sC, sH, sW) in elements."""
    if plane.dim() != 4 or plane.shape[0] != 1:
        raise RuntimeError(f'{name} must be [1,C,H,W]')
    if not plane.is_cuda:
        raise RuntimeError(f'{name} must be a CUDA tensor')
    check_f32(plane, name)
    _, _, H, W = plane.shape
    _, sC, sH, sW = plane.stride()
    return H, W, sC, sH, sW


def _plane_list(planes):
    if isinstance(planes, dict) or hasattr(planes, 'keys'):
        return [planes[k] for k in PLANE_KEYS]
    planes = list(planes)
    if len(planes) != 3:
        raise ValueError("planes: a dict with the keys 'xy', 'yz', 'zx' or a sequence of three")
    return planes


def _plane_pack(planes):
    """the three planes -> the flat [tensor, H, W, sC, sH, sW] * 3 every plane entry point of the library takes"""
    pack = []
    for p, k in zip(planes, PLANE_KEYS):
        pack += [p, *_plane_geom(p, k)]
    return pack


def _check_aggregation(aggregation):
    if aggregation not in ('concat', 'sum'):
        raise ValueError(f"aggregation must be 'concat' or 'sum', got {aggregation!r}")


def _is_channels_last(p):
    return p.stride(1) == 1 or p.shape[1] == 1


def _kernel_tensors(ctx, tensors, M):
    """The forward half of the plane ops' autograd functions: the relayout rule (TRIPLANE_RELAYOUT), keyed on the three
    planes that lead `tensors`, for M samples.  Records on ctx which tensors the kernel gets as channels-last copies
    (ctx.relayout) and the tensors themselves (ctx.meta), and returns what the kernel gets."""
    relayout = TRIPLANE_RELAYOUT and M >= max(p.shape[2] * p.shape[3] for p in tensors[:3])
    ctx.relayout = [relayout and not _is_channels_last(t) for t in tensors]
    ctx.meta = tensors
    return [t.contiguous(memory_format=torch.channels_last) if r else t for t, r in zip(tensors, ctx.relayout)]


def _scatter_grads(ctx, needs, scatter):
    """The backward half: zero-filled buffers with the strides of each tensor of ctx.meta (or channels-last where the kernel
    was handed a copy), `scatter(buffers)` -- one launch into all of them, so a tensor that wants no gradient still gets a
    buffer -- and None for the tensors that `needs` says want none."""
    if not any(needs):
        return [None] * len(needs)
    grads = [torch.zeros_like(t, memory_format=torch.channels_last if r else torch.preserve_format)
             for t, r in zip(ctx.meta, ctx.relayout)]
    scatter(grads)
    return [g if need else None for g, need in zip(grads, needs)]


def triplane_fwd(planes, xyz, xyz_min, xyz_max, aggregation='concat'):
    """dvgo_triplane_fwd on the planes' strides as they are: xyz [M,3] -> [M,3C] (concat) or [M,C] (sum).  No autograd."""
    _check_aggregation(aggregation)
    planes = _plane_list(planes)
    pack = _plane_pack(planes)
    C = planes[0].shape[1]
    if any(p.shape[1] != C for p in planes):
        raise RuntimeError('the three planes must share their channel count')
    check_input(xyz, 'xyz'); check_f32(xyz, 'xyz')
    M = xyz.shape[0]
    out = torch.empty((M, C if aggregation == 'sum' else 3 * C), dtype=torch.float32, device=xyz.device)
    with L.device_of(xyz):
        L.call('dvgo_triplane_fwd', *pack, C, xyz, xyz_min, xyz_max, M, 1 if aggregation == 'sum' else 0, out, stream_of(xyz))
    return out


def triplane_bwd(grad_out, grads, xyz, xyz_min, xyz_max, aggregation='concat', run=0):
    """dvgo_triplane_bwd: accumulates into the three buffers `grads` (shaped and strided like planes) in place.
    `run`: samples a lane merges before its atomics (0: the library's default)."""
    grads = _plane_list(grads)
    pack = _plane_pack(grads)
    C = grads[0].shape[1]
    check_input(grad_out, 'grad_out'); check_f32(grad_out, 'grad_out')
    M = xyz.shape[0]
    if tuple(grad_out.shape) != (M, C if aggregation == 'sum' else 3 * C):
        raise RuntimeError('grad_out has the wrong shape')
    with L.device_of(xyz):
        L.call('dvgo_triplane_bwd', grad_out, *pack, C, xyz, xyz_min, xyz_max, M, 1 if aggregation == 'sum' else 0, int(run),
               stream_of(xyz))
    return grads


class _TriPlaneSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xy, yz, zx, xyz, xyz_min, xyz_max, aggregation):
        out = triplane_fwd(_kernel_tensors(ctx, [xy, yz, zx], xyz.shape[0]), xyz, xyz_min, xyz_max, aggregation)
        ctx.save_for_backward(xyz, xyz_min, xyz_max)
        ctx.aggregation = aggregation
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        xyz, xyz_min, xyz_max = ctx.saved_tensors
        grads = _scatter_grads(ctx, ctx.needs_input_grad[:3],
                               lambda g: triplane_bwd(grad_out.contiguous(), g, xyz, xyz_min, xyz_max, ctx.aggregation))
        return (*grads, None, None, None, None)


def triplane_sample(planes, xyz, xyz_min, xyz_max, aggregation='concat'):
    """The reference's grid_sampler2D (lib/tri_dvgo.py:456-469) as one HIP op: `planes` is a dict with the keys 'xy',
    'yz', 'zx' (or the three in that order), each [1,C,H,W] float32 of any size and dense layout; xyz [...,3] world
    coordinates -> [...,3C] ('concat': xy, yz, zx) or [...,C] ('sum': (xy + yz) + zx).  Plane xy has its rows along world
    y and its columns along z, yz rows x / columns y, zx rows z / columns x (the reference's flipped ind_norm).
    Differentiable w.r.t. the planes only."""
    _check_aggregation(aggregation)
    xy, yz, zx = _plane_list(planes)
    for p, k in zip((xy, yz, zx), PLANE_KEYS):
        _plane_geom(p, k)
    shape = xyz.shape[:-1]
    flat = xyz.reshape(-1, 3).contiguous()
    out = _TriPlaneSample.apply(xy, yz, zx, flat, xyz_min.contiguous(), xyz_max.contiguous(), aggregation)
    return out.reshape(*shape, out.shape[-1])


# ---------------------------------------------------------------------------------------------- VM decomposition
def _line_geom(line, name):
    """line [1,R,N,1] (any dense strides) -> (N, sC, sN) in elements."""
    if line.dim() != 4 or line.shape[0] != 1 or line.shape[3] != 1:
        raise RuntimeError(f'{name} must be [1,R,N,1]')
    if not line.is_cuda:
        raise RuntimeError(f'{name} must be a CUDA tensor')
    check_f32(line, name)
    return line.shape[2], line.stride(1), line.stride(2)


def _vm_geom(tensors):
    """The three planes, then the three lines, of a VM kernel -> (its 30 plane-and-line arguments: each tensor followed by
    its geometry scalars, in call order; R)"""
    planes, lines = list(tensors[:3]), list(tensors[3:])
    R = planes[0].shape[1]
    if any(t.dim() != 4 or t.shape[1] != R for t in planes + lines):
        raise RuntimeError('the three planes [1,R,H,W] and the three lines [1,R,N,1] must share their component count')
    geom = _plane_pack(planes)
    for ln, k in zip(lines, PLANE_KEYS):
        geom += [ln, *_line_geom(ln, k + '_line')]
    assert len(geom) == 30              # (callers splat it into launches whose other arguments tests/test_abi.py counts)
    return geom, R


def _vm_args(planes, lines, xyz):
    """-> (planes, lines, `_vm_geom`'s argument list, R, M)"""
    planes, lines = _plane_list(planes), _plane_list(lines)
    geom, R = _vm_geom(planes + lines)
    check_input(xyz, 'xyz'); check_f32(xyz, 'xyz')
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise RuntimeError('xyz must be [M,3]')
    return planes, lines, geom, R, xyz.shape[0]


def _vm_tensors(planes, lines):
    """The checks of `vm_sample` and `vm_density` ahead of their autograd functions -> the three planes, then the three lines."""
    tensors = _plane_list(planes) + _plane_list(lines)
    for ln, k in zip(tensors[3:], PLANE_KEYS):             # shapes before devices
        if ln.dim() != 4 or ln.shape[0] != 1 or ln.shape[3] != 1:
            raise RuntimeError(f'{k}_line must be [1,R,N,1]')
    for p, k in zip(tensors[:3], PLANE_KEYS):
        _plane_geom(p, k)
    for ln, k in zip(tensors[3:], PLANE_KEYS):
        _line_geom(ln, k + '_line')
    return tensors


def _vm_grad_args(tensors, grad_planes, grad_lines):
    """The six gradient buffers of `vm_bwd` and `vm_density_bwd`, checked against the planes and lines they belong to."""
    grad_planes, grad_lines = _plane_list(grad_planes), _plane_list(grad_lines)
    for t, g in zip(tensors, grad_planes + grad_lines):
        if g.shape != t.shape or g.dtype != torch.float32 or g.device != t.device or \
                any(a != b for a, b, n in zip(g.stride(), t.stride(), t.shape) if n > 1):
            raise RuntimeError('a gradient buffer must have the shape, strides, dtype and device of the tensor it belongs to')
    return grad_planes, grad_lines


def vm_fwd(planes, lines, xyz, xyz_min, xyz_max):
    """dvgo_vm_fwd on the strides as they are: planes [1,R,H,W], lines [1,R,N,1], xyz [M,3] -> [M,3R], plane value times
    line value per component (xy, yz, zx; include/dvgo_hip.h has the arithmetic).  No autograd."""
    planes, lines, geom, R, M = _vm_args(planes, lines, xyz)
    out = torch.empty((M, 3 * R), dtype=torch.float32, device=xyz.device)
    with L.device_of(xyz):
        L.call('dvgo_vm_fwd', *geom, R, xyz, xyz_min, xyz_max, M, out, stream_of(xyz))
    return out


def vm_bwd(grad_out, planes, lines, grad_planes, grad_lines, xyz, xyz_min, xyz_max, run=0, mode=0):
    """dvgo_vm_bwd: accumulates into the six buffers `grad_planes` / `grad_lines` (shaped and strided like the planes and
    lines they belong to) in place.  `run`: samples a lane merges before its atomics; `mode`: 1 all sums to global memory,
    2 the line sums through a table in LDS (0: the library's choice, for both)."""
    planes, lines, geom, R, M = _vm_args(planes, lines, xyz)
    grad_planes, grad_lines = _vm_grad_args(planes + lines, grad_planes, grad_lines)
    check_input(grad_out, 'grad_out'); check_f32(grad_out, 'grad_out')
    if tuple(grad_out.shape) != (M, 3 * R):
        raise RuntimeError('grad_out has the wrong shape')
    with L.device_of(xyz):
        L.call('dvgo_vm_bwd', grad_out, *geom, *grad_planes, *grad_lines, R, xyz, xyz_min, xyz_max, M, int(run), int(mode),
               stream_of(xyz))
    return grad_planes, grad_lines


def _vm_bwd_xyz(entry, per_comp, grad_out, planes, lines, xyz, xyz_min, xyz_max):
    planes, lines, geom, R, M = _vm_args(planes, lines, xyz)
    check_input(grad_out, 'grad_out'); check_f32(grad_out, 'grad_out')
    if tuple(grad_out.shape) != ((M, 3 * R) if per_comp else (M,)):
        raise RuntimeError('grad_out has the wrong shape')
    grad_xyz = torch.empty_like(xyz)
    with L.device_of(xyz):
        L.call(entry, *geom, R, grad_out, xyz, xyz_min, xyz_max, M, grad_xyz, stream_of(xyz))
    return grad_xyz


def vm_bwd_xyz(grad_out, planes, lines, xyz, xyz_min, xyz_max):
    """dvgo_vm_bwd_xyz: the gradient of `vm_fwd`'s features with respect to the positions, grad_out [M, 3R], xyz [M,3] ->
    [M,3], every row written (csrc/vm_xyz.hip; include/dvgo_hip.h has the arithmetic).  No autograd."""
    return _vm_bwd_xyz('dvgo_vm_bwd_xyz', True, grad_out, planes, lines, xyz, xyz_min, xyz_max)


def vm_density_bwd_xyz(grad_out, planes, lines, xyz, xyz_min, xyz_max):
    """dvgo_vm_density_bwd_xyz: `vm_bwd_xyz` for `vm_density_fwd`, one float of incoming gradient per sample, grad_out [M];
    a sample whose gradient is exactly 0 gets an exactly zero row.  No autograd."""
    return _vm_bwd_xyz('dvgo_vm_density_bwd_xyz', False, grad_out, planes, lines, xyz, xyz_min, xyz_max)


class _VMSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, xyz_min, xyz_max, *tensors):
        kt = _kernel_tensors(ctx, tensors, xyz.shape[0])           # the rule looks at the three planes only
        out = vm_fwd(kt[:3], kt[3:], xyz, xyz_min, xyz_max)
        ctx.save_for_backward(xyz, xyz_min, xyz_max, *kt)          # the gradient of a product reads the other factor
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        xyz, xyz_min, xyz_max, *kt = ctx.saved_tensors
        grad_xyz = None
        grad_out = grad_out.contiguous()
        # the position kernel first, the scatter after it (_HashSample.backward states the rule); it reads the saved `kt`
        # the forward read
        if ctx.needs_input_grad[0]:
            grad_xyz = vm_bwd_xyz(grad_out, kt[:3], kt[3:], xyz, xyz_min, xyz_max)
        grads = _scatter_grads(ctx, ctx.needs_input_grad[3:],
                               lambda g: vm_bwd(grad_out, kt[:3], kt[3:], g[:3], g[3:], xyz, xyz_min, xyz_max))
        return (grad_xyz, None, None, *grads)


def vm_sample(planes, lines, xyz, xyz_min, xyz_max, position_grad=False):
    """TensoRF's vector-matrix features as one HIP op: `planes` as in `triplane_sample`, each [1,R,H,W]; `lines` likewise a
    dict with the keys 'xy', 'yz', 'zx' (or the three in that order), each [1,R,N,1], line s running along the world axis
    plane s does not see (xy: x, yz: z, zx: y); xyz [...,3] world coordinates -> [...,3R]: per component the plane's
    bilinear value times the line's linear value, in the order xy, yz, zx.  Differentiable w.r.t. planes and lines and, with
    `position_grad=True` and an `xyz` that requires grad, w.r.t. `xyz` (csrc/vm_xyz.hip: the derivative of the cell the
    forward chose, with the forward's zero padding; once differentiable).  The forward is the same launch either way; by
    default `xyz` is detached."""
    tensors = _vm_tensors(planes, lines)
    shape = xyz.shape[:-1]
    flat = (xyz if position_grad else xyz.detach()).reshape(-1, 3).contiguous()
    out = _VMSample.apply(flat, xyz_min.contiguous(), xyz_max.contiguous(), *tensors)
    return out.reshape(*shape, out.shape[-1])


def vm_density_fwd(planes, lines, xyz, xyz_min, xyz_max):
    """dvgo_vm_density_fwd on the strides as they are: planes [1,R,H,W], lines [1,R,N,1], xyz [M,3] -> [M], the sum of
    `vm_fwd`'s 3R products as one fma chain in the order xy, yz, zx, component upwards (include/dvgo_hip.h).  No autograd."""
    planes, lines, g, R, M = _vm_args(planes, lines, xyz)
    out = torch.empty((M,), dtype=torch.float32, device=xyz.device)
    with L.device_of(xyz):
        L.call('dvgo_vm_density_fwd', *g, R, xyz, xyz_min, xyz_max, M, out, stream_of(xyz))
    return out


def vm_density_bwd(grad_out, planes, lines, grad_planes, grad_lines, xyz, xyz_min, xyz_max, run=0, mode=0):
    """dvgo_vm_density_bwd: `vm_bwd` with one float of incoming gradient per sample, grad_out [M]; samples whose gradient
    is exactly 0 are passed over.  Accumulates into the six buffers in place; `run` and `mode` as in `vm_bwd`."""
    planes, lines, g, R, M = _vm_args(planes, lines, xyz)
    gp, gl = _vm_grad_args(planes + lines, grad_planes, grad_lines)
    check_input(grad_out, 'grad_out'); check_f32(grad_out, 'grad_out')
    if tuple(grad_out.shape) != (M,):
        raise RuntimeError('grad_out has the wrong shape')
    with L.device_of(xyz):
        L.call('dvgo_vm_density_bwd', grad_out, *g, *gp, *gl, R, xyz, xyz_min, xyz_max, M, int(run), int(mode), stream_of(xyz))
    return gp, gl


def _vm_grad_buffers(kt):
    """Zero-filled gradient buffers for the six tensors `kt` a VM kernel read, each with its tensor's shape and strides:
    `_scatter_grads` with one zero fill instead of six -- views of one allocation (256-byte aligned).  On a sparse batch the
    backward is bound by its launches, not by the scatter (profiles/vm_density/README.md)."""
    if not all(t.is_contiguous() or t.is_contiguous(memory_format=torch.channels_last) for t in kt):
        return [torch.zeros_like(t, memory_format=torch.preserve_format) for t in kt]
    offs, top = [], 0
    for t in kt:
        offs.append(top)
        top += (t.numel() + 63) // 64 * 64
    flat = torch.zeros(top, dtype=torch.float32, device=kt[0].device)
    return [flat.as_strided(t.shape, t.stride(), o) for t, o in zip(kt, offs)]


class _VMDensity(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, xyz_min, xyz_max, *tensors):
        kt = _kernel_tensors(ctx, tensors, xyz.shape[0])           # the rule looks at the three planes only
        out = vm_density_fwd(kt[:3], kt[3:], xyz, xyz_min, xyz_max)
        ctx.save_for_backward(xyz, xyz_min, xyz_max, *kt)          # the gradient of a product reads the other factor
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        xyz, xyz_min, xyz_max, *kt = ctx.saved_tensors
        needs = ctx.needs_input_grad[3:]
        grad_xyz = None
        grad_out = grad_out.contiguous()
        # the position kernel first, the scatter after it (_HashSample.backward states the rule); it reads the saved `kt`
        # the forward read
        if ctx.needs_input_grad[0]:
            grad_xyz = vm_density_bwd_xyz(grad_out, kt[:3], kt[3:], xyz, xyz_min, xyz_max)
        if not any(needs):
            return (grad_xyz,) + (None,) * 8
        grads = _vm_grad_buffers(kt)
        vm_density_bwd(grad_out, kt[:3], kt[3:], grads[:3], grads[3:], xyz, xyz_min, xyz_max)
        return (grad_xyz, None, None, *[g if need else None for g, need in zip(grads, needs)])


def vm_density(planes, lines, xyz, xyz_min, xyz_max, position_grad=False):
    """TensoRF's vector-matrix density as one HIP op: `planes` and `lines` as in `vm_sample`; xyz [...,3] world coordinates
    -> [...]: the sum over the three planes and their R components of plane value times line value, summed on chip (no
    [M, 3R] intermediate, forward or backward).  Differentiable w.r.t. planes and lines and, with `position_grad=True` and
    an `xyz` that requires grad, w.r.t. `xyz` (csrc/vm_xyz.hip, as in `vm_sample`).  The forward is the same launch either
    way; by default `xyz` is detached."""
    tensors = _vm_tensors(planes, lines)
    shape = xyz.shape[:-1]
    flat = (xyz if position_grad else xyz.detach()).reshape(-1, 3).contiguous()
    return _VMDensity.apply(flat, xyz_min.contiguous(), xyz_max.contiguous(), *tensors).reshape(shape)


# ---------------------------------------------------------------------------------------------- hash grid
HASH_MAX_LEVELS = 32                     # DVGO_HASH_MAX_LEVELS


class HashLevels:
    """The level table of a hash grid as the library takes it: `res` [L,3] node counts and `offsets` [L+1] first rows, kept
    as host arrays.  Checked here with the library's own rule, so a bad table is a ValueError before anything is launched."""

    def __init__(self, res, offsets):
        res = torch.as_tensor(res).detach().cpu().to(torch.int64).reshape(-1, 3)
        offsets = torch.as_tensor(offsets).detach().cpu().to(torch.int64).reshape(-1)
        L_ = res.shape[0]
        if not 1 <= L_ <= HASH_MAX_LEVELS or offsets.numel() != L_ + 1:
            raise ValueError(f'res must be [L,3] and offsets [L+1] with 1 <= L <= {HASH_MAX_LEVELS}, got {tuple(res.shape)} and '
                             f'{tuple(offsets.shape)}')
        self.res, self.offsets = res.tolist(), offsets.tolist()
        if self.offsets[0] < 0:
            raise ValueError('offsets[0] must not be negative')
        self.hashed = []
        for l, (r, a, b) in enumerate(zip(self.res, self.offsets[:-1], self.offsets[1:])):
            nodes, size = r[0] * r[1] * r[2], b - a
            if min(r) < 2 or max(r) >= 2 ** 31:
                raise ValueError(f'level {l}: every node count must be at least 2 (and below 2^31), got {r}')
            if size != nodes and (size < 1 or size > nodes or size & (size - 1)):
                raise ValueError(f'level {l}: {size} rows for {r[0]} x {r[1]} x {r[2]} = {nodes} nodes: a level has one row per '
                                 'node (dense) or a power of two below that (hashed)')
            self.hashed.append(size != nodes)
        self.L, self.rows = L_, self.offsets[-1]
        self.c_res = (ctypes.c_int32 * (3 * L_))(*[v for r in self.res for v in r])
        self.c_offsets = (ctypes.c_int64 * (L_ + 1))(*self.offsets)


def _hash_args(table, levels, xyz, name='table'):
    if table.dim() != 2 or table.shape[1] not in (1, 2, 4, 8):
        raise ValueError(f'{name} must be [T, F] with F in (1, 2, 4, 8), got {tuple(table.shape)}')
    if table.shape[0] < levels.rows:
        raise ValueError(f'{name} has {table.shape[0]} rows, the level table addresses {levels.rows}')
    check_input(table, name); check_f32(table, name)
    check_input(xyz, 'xyz'); check_f32(xyz, 'xyz')
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise RuntimeError('xyz must be [M,3]')
    return table.shape[1], xyz.shape[0]


def hash_fwd(table, xyz, xyz_min, xyz_max, levels):
    """dvgo_hash_fwd: table [T,F], xyz [M,3], `levels` a HashLevels -> [M, L F] (include/dvgo_hip.h has the arithmetic).
    No autograd."""
    Fc, M = _hash_args(table, levels, xyz)
    out = torch.empty((M, levels.L * Fc), dtype=torch.float32, device=xyz.device)
    with L.device_of(xyz):
        L.call('dvgo_hash_fwd', table, Fc, levels.L, levels.c_res, levels.c_offsets, xyz, xyz_min, xyz_max, M, out, stream_of(xyz))
    return out


def hash_bwd(grad_out, grad_table, xyz, xyz_min, xyz_max, levels, run=0, mode=0):
    """dvgo_hash_bwd: accumulates into the buffer `grad_table` (shaped like the table) in place.  `mode` 1: a lane merges
    `run` consecutive samples of a level while they stay in one cell; 3: the same with one lane per channel; 2: nothing
    merged (0: the library's choice, for both)."""
    Fc, M = _hash_args(grad_table, levels, xyz, 'grad_table')
    check_input(grad_out, 'grad_out'); check_f32(grad_out, 'grad_out')
    if tuple(grad_out.shape) != (M, levels.L * Fc):
        raise RuntimeError('grad_out has the wrong shape')
    with L.device_of(xyz):
        L.call('dvgo_hash_bwd', grad_out, grad_table, Fc, levels.L, levels.c_res, levels.c_offsets, xyz, xyz_min, xyz_max, M,
               int(run), int(mode), stream_of(xyz))
    return grad_table


def hash_bwd_xyz(table, grad_out, xyz, xyz_min, xyz_max, levels):
    """dvgo_hash_bwd_xyz: the gradient of the features with respect to the positions, table [T,F], grad_out [M, L F],
    xyz [M,3] -> [M,3], every row written (include/dvgo_hip.h has the arithmetic).  No autograd."""
    Fc, M = _hash_args(table, levels, xyz)
    check_input(grad_out, 'grad_out'); check_f32(grad_out, 'grad_out')
    if tuple(grad_out.shape) != (M, levels.L * Fc):
        raise RuntimeError('grad_out has the wrong shape')
    grad_xyz = torch.empty_like(xyz)
    with L.device_of(xyz):
        L.call('dvgo_hash_bwd_xyz', table, Fc, levels.L, levels.c_res, levels.c_offsets, grad_out, xyz, xyz_min, xyz_max, M,
               grad_xyz, stream_of(xyz))
    return grad_xyz


class _HashSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, xyz, xyz_min, xyz_max, levels):
        out = hash_fwd(table, xyz, xyz_min, xyz_max, levels)
        if ctx.needs_input_grad[1]:       # the position gradient reads the table's values
            ctx.save_for_backward(xyz, xyz_min, xyz_max, table)
        else:                             # linear in the table: its values are not needed again
            ctx.save_for_backward(xyz, xyz_min, xyz_max)
        ctx.levels, ctx.shape = levels, table.shape
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        xyz, xyz_min, xyz_max = ctx.saved_tensors[:3]
        grad = grad_xyz = None
        grad_out = grad_out.contiguous()
        # the position kernel first: it reads the table's values, which an in-place optimizer step may change
        # (_FusedMarch.backward states the rule); the scatter after it, on the same stream, reads none
        if ctx.needs_input_grad[1]:
            grad_xyz = hash_bwd_xyz(ctx.saved_tensors[3], grad_out, xyz, xyz_min, xyz_max, ctx.levels)
        if ctx.needs_input_grad[0]:
            grad = torch.zeros(ctx.shape, dtype=torch.float32, device=xyz.device)
            hash_bwd(grad_out, grad, xyz, xyz_min, xyz_max, ctx.levels)
        return grad, grad_xyz, None, None, None


def hash_sample(table, xyz, xyz_min, xyz_max, res, offsets=None, position_grad=False):
    """Multiresolution hash-grid features (Instant-NGP) as one HIP op: `table` [T_total, F] float32 contiguous, F in
    (1, 2, 4, 8); `res` [L,3] the node counts of every level along x, y, z and `offsets` [L+1] the levels' first rows (host
    values: tensors, arrays or lists), or `res` a HashLevels made from them once; xyz [...,3] world coordinates ->
    [..., L F], level by level.  A level with one row per node is dense, any other is hashed into its power-of-two row
    count; a table that fits neither is a ValueError.  Positions outside the box read its faces.  Differentiable w.r.t.
    `table` and, with `position_grad=True` and an `xyz` that requires grad, w.r.t. `xyz` (csrc/hash_xyz.hip: the derivative
    of the cell the forward chose, zero along an axis on which the position lies outside the box; once differentiable; the
    table is then saved for the backward).  The forward is the same launch either way; by default `xyz` is detached."""
    levels = res if isinstance(res, HashLevels) else HashLevels(res, offsets)
    shape = xyz.shape[:-1]
    flat = (xyz if position_grad else xyz.detach()).reshape(-1, 3).contiguous()
    _hash_args(table, levels, flat)
    out = _HashSample.apply(table, flat, xyz_min.contiguous(), xyz_max.contiguous(), levels)
    return out.reshape(*shape, out.shape[-1])


# ---------------------------------------------------------------------------------------------- LIIF plane decoder
def _liif_args(planes, xyz, world_size):
    """-> (planes, their _plane_pack, C, M, (Wx, Wy, Wz))"""
    planes = _plane_list(planes)
    pack = _plane_pack(planes)
    C = planes[0].shape[1]
    if any(p.shape[1] != C for p in planes):
        raise RuntimeError('the three planes must share their channel count')
    check_input(xyz, 'xyz'); check_f32(xyz, 'xyz')
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise RuntimeError('xyz must be [M,3]')
    ws = tuple(int(v) for v in world_size)
    if len(ws) != 3 or min(ws) < 1:
        raise ValueError(f'world_size must be three extents >= 1, got {ws}')
    return planes, pack, C, xyz.shape[0], ws


def liif_gather_fwd(planes, xyz, xyz_min, xyz_max, world_size, cell_decode=True, local_ensemble=True):
    """dvgo_liif_gather on the planes' strides as they are: xyz [M,3] -> inp [3,E,M,D], wgt [3,E,M] (E = 4 with
    local_ensemble, else 1; D = C + 4 with cell_decode, else C + 2).  No autograd."""
    planes, pack, C, M, ws = _liif_args(planes, xyz, world_size)
    E, D = (4 if local_ensemble else 1), C + (4 if cell_decode else 2)
    inp = torch.empty((3, E, M, D), dtype=torch.float32, device=xyz.device)
    wgt = torch.empty((3, E, M), dtype=torch.float32, device=xyz.device)
    with L.device_of(xyz):
        L.call('dvgo_liif_gather', *pack, C, xyz, xyz_min, xyz_max, M, *ws, int(bool(cell_decode)), int(bool(local_ensemble)),
               inp, wgt, stream_of(xyz))
    return inp, wgt


def liif_gather_bwd(grad_inp, grads, xyz, xyz_min, xyz_max, world_size, cell_decode=True, local_ensemble=True, run=0):
    """dvgo_liif_scatter: accumulates the first C columns of grad_inp [3,E,M,D] into the three buffers `grads` (shaped
    and strided like planes) in place.  `run`: samples a lane merges before its atomic (0: the library's default)."""
    grads, pack, C, M, ws = _liif_args(grads, xyz, world_size)
    E, D = (4 if local_ensemble else 1), C + (4 if cell_decode else 2)
    check_input(grad_inp, 'grad_inp'); check_f32(grad_inp, 'grad_inp')
    if tuple(grad_inp.shape) != (3, E, M, D):
        raise RuntimeError('grad_inp has the wrong shape')
    with L.device_of(xyz):
        L.call('dvgo_liif_scatter', grad_inp, *pack, C, xyz, xyz_min, xyz_max, M, *ws, int(bool(cell_decode)),
               int(bool(local_ensemble)), int(run), stream_of(xyz))
    return grads


def _blend_shape(pred, wgt):
    check_input(pred, 'pred'); check_f32(pred, 'pred'); check_input(wgt, 'wgt'); check_f32(wgt, 'wgt')
    if pred.dim() != 4 or pred.shape[0] != 3 or pred.shape[1] not in (1, 4) or tuple(wgt.shape) != tuple(pred.shape[:3]):
        raise RuntimeError('pred must be [3,E,M,C] with E = 1 or 4 and wgt [3,E,M]')
    return pred.shape[1:]


def liif_blend_fwd(pred, wgt, aggregation='concat'):
    """dvgo_liif_blend_fwd: pred [3,E,M,C], wgt [3,E,M] -> [M,3C] (concat) or [M,C] (sum).  No autograd."""
    _check_aggregation(aggregation)
    E, M, C = _blend_shape(pred, wgt)
    out = torch.empty((M, C if aggregation == 'sum' else 3 * C), dtype=torch.float32, device=pred.device)
    with L.device_of(pred):
        L.call('dvgo_liif_blend_fwd', pred, wgt, C, M, E, 1 if aggregation == 'sum' else 0, out, stream_of(pred))
    return out


def liif_blend_bwd(grad_out, wgt, C, aggregation='concat'):
    """dvgo_liif_blend_bwd: grad_out [M,3C] or [M,C], wgt [3,E,M] -> grad_pred [3,E,M,C]."""
    check_input(grad_out, 'grad_out'); check_f32(grad_out, 'grad_out'); check_input(wgt, 'wgt'); check_f32(wgt, 'wgt')
    _, E, M = wgt.shape
    if tuple(grad_out.shape) != (M, C if aggregation == 'sum' else 3 * C):
        raise RuntimeError('grad_out has the wrong shape')
    grad_pred = torch.empty((3, E, M, C), dtype=torch.float32, device=wgt.device)
    with L.device_of(wgt):
        L.call('dvgo_liif_blend_bwd', grad_out, wgt, C, M, E, 1 if aggregation == 'sum' else 0, grad_pred, stream_of(wgt))
    return grad_pred


class _LiifGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xy, yz, zx, xyz, xyz_min, xyz_max, world_size, cell_decode, local_ensemble):
        inp, wgt = liif_gather_fwd(_kernel_tensors(ctx, [xy, yz, zx], xyz.shape[0]), xyz, xyz_min, xyz_max, world_size, cell_decode,
                                   local_ensemble)
        ctx.save_for_backward(xyz, xyz_min, xyz_max)
        ctx.geometry = (world_size, cell_decode, local_ensemble)
        ctx.mark_non_differentiable(wgt)
        return inp, wgt

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_inp, _grad_wgt):
        xyz, xyz_min, xyz_max = ctx.saved_tensors
        grads = _scatter_grads(ctx, ctx.needs_input_grad[:3],
                               lambda g: liif_gather_bwd(grad_inp.contiguous(), g, xyz, xyz_min, xyz_max, *ctx.geometry))
        return (*grads, None, None, None, None, None, None)


class _LiifBlend(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, wgt, aggregation):
        ctx.save_for_backward(wgt)
        ctx.aggregation, ctx.C = aggregation, pred.shape[3]
        return liif_blend_fwd(pred, wgt, aggregation)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        wgt, = ctx.saved_tensors
        return liif_blend_bwd(grad_out.contiguous(), wgt, ctx.C, ctx.aggregation), None, None


def liif_gather(planes, xyz, xyz_min, xyz_max, world_size, cell_decode=True, local_ensemble=True):
    """The gathers of the reference's liif_interpolate (lib/tri_dvgo.py:481-565) as one HIP op: planes as in
    `triplane_sample`, xyz [M,3] -> (inp [3,E,M,D], wgt [3,E,M]): per plane (xy, yz, zx) and shifted position the MLP input
    rows [nearest texel's C features, rel0, rel1(, cell0, cell1)] and the blend weights (include/dvgo_hip.h has the
    arithmetic).  Differentiable w.r.t. the planes only, through the feature columns; wgt carries no gradient."""
    xy, yz, zx = _plane_list(planes)
    for p, k in zip((xy, yz, zx), PLANE_KEYS):
        _plane_geom(p, k)
    ws = tuple(int(v) for v in world_size)
    return _LiifGather.apply(xy, yz, zx, xyz.reshape(-1, 3).contiguous(), xyz_min.contiguous(), xyz_max.contiguous(), ws,
                             bool(cell_decode), bool(local_ensemble))


def liif_blend(pred, wgt, aggregation='concat'):
    """pred [3,E,M,C] blended over the shifts by wgt [3,E,M] and aggregated over the planes: [M,3C] ('concat') or [M,C]
    ('sum': (xy + yz) + zx).  Differentiable w.r.t. pred only."""
    _check_aggregation(aggregation)
    return _LiifBlend.apply(pred.contiguous(), wgt, aggregation)


def liif_decode(planes, nets, xyz, xyz_min, xyz_max, world_size, cell_decode=True, local_ensemble=True, aggregation='concat'):
    """liif_interpolate: gather, the decoders, blend.  `nets`: {'xy': module, 'yz': module}; plane zx is decoded by
    nets['yz'] as in the reference (lib/tri_dvgo.py:170-174), so the MLPs run twice -- once on the E*M rows of plane xy,
    once on the 2*E*M rows of planes yz and zx -- instead of 3 E times."""
    inp, wgt = liif_gather(planes, xyz, xyz_min, xyz_max, world_size, cell_decode, local_ensemble)
    _, E, M, D = inp.shape
    pred = torch.cat([nets['xy'](inp[0].reshape(E * M, D)), nets['yz'](inp[1:].reshape(2 * E * M, D))])
    return liif_blend(pred.reshape(3, E, M, -1), wgt, aggregation)


# ---------------------------------------------------------------------------------------------- bilinear plane decoder
def _rows_width(C, n_freq, cell_decode):
    n_freq = int(n_freq)
    if n_freq < 1:
        raise ValueError(f'n_freq must be at least 1, got {n_freq}')
    return n_freq, C + 2 + 4 * n_freq + (2 if cell_decode else 0)


def plane_rows_fwd(planes, xyz, xyz_min, xyz_max, world_size, n_freq, cell_decode=True):
    """dvgo_plane_rows_fwd on the planes' strides as they are: xyz [M,3] -> inp [3,M,D], D = C + 2 + 4 * n_freq (+ 2 with
    cell_decode).  No autograd."""
    planes, pack, C, M, ws = _liif_args(planes, xyz, world_size)
    P, D = _rows_width(C, n_freq, cell_decode)
    inp = torch.empty((3, M, D), dtype=torch.float32, device=xyz.device)
    with L.device_of(xyz):
        L.call('dvgo_plane_rows_fwd', *pack, C, xyz, xyz_min, xyz_max, M, *ws, P, int(bool(cell_decode)), inp, stream_of(xyz))
    return inp


def plane_rows_bwd(grad_inp, grads, xyz, xyz_min, xyz_max, world_size, n_freq, cell_decode=True, run=0):
    """dvgo_plane_rows_bwd: accumulates w * (the first C columns of grad_inp [3,M,D]) into the three buffers `grads` (shaped
    and strided like planes) in place.  `run`: samples a lane merges before its atomics (0: the library's default)."""
    grads, pack, C, M, ws = _liif_args(grads, xyz, world_size)
    P, D = _rows_width(C, n_freq, cell_decode)
    check_input(grad_inp, 'grad_inp'); check_f32(grad_inp, 'grad_inp')
    if tuple(grad_inp.shape) != (3, M, D):
        raise RuntimeError('grad_inp has the wrong shape')
    with L.device_of(xyz):
        L.call('dvgo_plane_rows_bwd', grad_inp, *pack, C, xyz, xyz_min, xyz_max, M, *ws, P, int(bool(cell_decode)), int(run),
               stream_of(xyz))
    return grads


class _PlaneRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xy, yz, zx, xyz, xyz_min, xyz_max, world_size, n_freq, cell_decode):
        inp = plane_rows_fwd(_kernel_tensors(ctx, [xy, yz, zx], xyz.shape[0]), xyz, xyz_min, xyz_max, world_size, n_freq, cell_decode)
        ctx.save_for_backward(xyz, xyz_min, xyz_max)
        ctx.geometry = (world_size, n_freq, cell_decode)
        return inp

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_inp):
        xyz, xyz_min, xyz_max = ctx.saved_tensors
        grads = _scatter_grads(ctx, ctx.needs_input_grad[:3],
                               lambda g: plane_rows_bwd(grad_inp.contiguous(), g, xyz, xyz_min, xyz_max, *ctx.geometry))
        return (*grads, None, None, None, None, None, None)


def plane_rows(planes, xyz, xyz_min, xyz_max, world_size, n_freq, cell_decode=True):
    """The samplers, the coordinate encoding and the cats of the reference's interpolate (lib/tri_dvgo.py:568-607) as one
    HIP op: planes as in `triplane_sample`, xyz [M,3] -> inp [3,M,D]: per plane (xy, yz, zx) the MLP input rows [C bilinear
    features, q0, q1, sin(q * 2^j), cos(q * 2^j)(, cell_a, cell_b)] (include/dvgo_hip.h has the arithmetic).  Differentiable
    w.r.t. the planes only, through the feature columns."""
    xy, yz, zx = _plane_list(planes)
    for p, k in zip((xy, yz, zx), PLANE_KEYS):
        _plane_geom(p, k)
    ws = tuple(int(v) for v in world_size)
    return _PlaneRows.apply(xy, yz, zx, xyz.reshape(-1, 3).contiguous(), xyz_min.contiguous(), xyz_max.contiguous(), ws,
                            int(n_freq), bool(cell_decode))


def interp_decode(planes, nets, xyz, xyz_min, xyz_max, world_size, n_freq, cell_decode=True, aggregation='concat'):
    """interpolate: rows, the decoders, aggregation.  `nets`: {'xy': module, 'yz': module}; plane zx is decoded by
    nets['yz'] as in the reference (lib/tri_dvgo.py:170-174), so the MLPs run twice -- once on the M rows of plane xy, once
    on the 2M rows of planes yz and zx.  -> [M, 3 * out] ('concat': xy, yz, zx) or [M, out] ('sum': (xy + yz) + zx)."""
    _check_aggregation(aggregation)
    inp = plane_rows(planes, xyz, xyz_min, xyz_max, world_size, n_freq, cell_decode)
    _, M, D = inp.shape
    p_xy = nets['xy'](inp[0])
    rest = nets['yz'](inp[1:].reshape(2 * M, D))
    p_yz, p_zx = rest.reshape(2, M, rest.shape[-1])         # the width named: -1 is ambiguous when no sample is kept
    if aggregation == 'concat':
        return torch.cat([p_xy, p_yz, p_zx], -1)
    return (p_xy + p_yz) + p_zx


class MaskCache(nn.Module):
    """Occupancy grid for free-space skipping (lib/dvgo.py:583-613).  ``path`` loads a coarse
    checkpoint ({'model_state_dict': {'density'}, 'model_kwargs': {...}}) exactly like the
    reference; otherwise ``mask`` + bbox are given."""

    def __init__(self, path=None, mask_cache_thres=None, mask=None, xyz_min=None, xyz_max=None):
        super().__init__()
        if path is not None:
            from .checkpoint import safe_load
            st = safe_load(path)                    # weights-only: nothing in the file is executed
            self.mask_cache_thres = mask_cache_thres
            density = F.max_pool3d(st['model_state_dict']['density'].float().contiguous(), kernel_size=3,
                                   padding=1, stride=1)
            kw = st['model_kwargs']
            alpha = 1 - torch.exp(-F.softplus(density + float(kw['act_shift'])) * float(kw['voxel_size_ratio']))
            mask = (alpha >= self.mask_cache_thres).squeeze(0).squeeze(0)
            xyz_min = torch.as_tensor(kw['xyz_min'], dtype=torch.float32)
            xyz_max = torch.as_tensor(kw['xyz_max'], dtype=torch.float32)
        else:
            mask = mask.bool()
            xyz_min = torch.as_tensor(xyz_min, dtype=torch.float32).detach().clone()
            xyz_max = torch.as_tensor(xyz_max, dtype=torch.float32).detach().clone()
        self.register_buffer('mask', mask.contiguous())
        xyz_len = xyz_max - xyz_min
        scale = (torch.tensor(list(mask.shape), dtype=torch.float32, device=xyz_len.device) - 1) / xyz_len
        self.register_buffer('xyz2ijk_scale', scale)
        self.register_buffer('xyz2ijk_shift', -xyz_min.to(scale.device) * scale)

    @torch.no_grad()
    def forward(self, xyz):
        shape = xyz.shape[:-1]
        xyz = xyz.reshape(-1, 3).contiguous()
        mask = render_utils_hip.maskcache_lookup(self.mask, xyz, self.xyz2ijk_scale, self.xyz2ijk_shift)
        return mask.reshape(shape)


class _SegmentSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, index, out):
        check_input(src, 'src'); check_input(index, 'index'); check_f32(src, 'src')
        if index.dtype != torch.int64:
            raise RuntimeError('index must be int64')
        squeeze = src.dim() == 1
        C = 1 if squeeze else src.shape[1]
        res = out.clone().contiguous()
        with L.device_of(src):
            L.call('dvgo_segment_sum', src, index, src.shape[0], C, res.shape[0], res, stream_of(src))
        ctx.save_for_backward(index)
        return res

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (index,) = ctx.saved_tensors
        return g.index_select(0, index), None, g   # d/d src = gather, d/d out = identity


def segment_coo(src, index, out, reduce='sum'):
    """torch_scatter.segment_coo(src, index, out, reduce='sum') as used at
    lib/dvgo.py:554-559,571-575: index sorted, out = zeros[N(,C)]; returns the summed tensor."""
    if reduce != 'sum':
        raise NotImplementedError("only reduce='sum' is used by the reference")
    return _SegmentSum.apply(src.contiguous(), index, out)


def ray_offsets(ray_id, N):
    """[N + 1] int64: where each ray's samples start in the sorted `ray_id` (what a fused march returns as off3)."""
    return torch.searchsorted(ray_id, torch.arange(N + 1, device=ray_id.device))


def _segment_sum3(src, ray_id, n):
    out = torch.zeros((n, 3), dtype=torch.float32, device=src.device)
    with L.device_of(src):
        L.call('dvgo_segment_sum', src, ray_id, src.shape[0], 3, n, out, stream_of(src))
    return out


class _RayPoints(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rays_o, rays_d, lam, ray_id, pts):
        for x, name in ((rays_o, 'rays_o'), (rays_d, 'rays_d'), (pts, 'pts'), (lam, 'lam')):
            check_input(x, name); check_f32(x, name)
        check_input(ray_id, 'ray_id')
        if ray_id.dtype != torch.int64:
            raise RuntimeError('ray_id must be int64')
        if pts.dim() != 2 or pts.shape[1] != 3 or lam.shape != ray_id.shape or lam.shape[0] != pts.shape[0]:
            raise RuntimeError('pts must be [M,3], lam and ray_id [M]')
        if rays_o.shape != rays_d.shape or rays_o.dim() != 2 or rays_o.shape[1] != 3:
            raise RuntimeError('rays_o and rays_d must be [N,3]')
        ctx.save_for_backward(lam, ray_id)
        ctx.n_rays = rays_o.shape[0]
        return pts.clone()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        lam, ray_id = ctx.saved_tensors
        g = g.contiguous()
        grad_o = _segment_sum3(g, ray_id, ctx.n_rays) if ctx.needs_input_grad[0] else None
        grad_d = _segment_sum3((lam.unsqueeze(-1) * g).contiguous(), ray_id, ctx.n_rays) if ctx.needs_input_grad[1] else None
        return grad_o, grad_d, None, None, None


def ray_points(rays_o, rays_d, lam, ray_id, pts):
    """The sampler's positions as a differentiable function of their rays.  Returns `pts` [M,3] unchanged, bit for bit
    (they are what the sampling kernel wrote), and states pts[m] = rays_o[ray_id[m]] + rays_d[ray_id[m]] * lam[m] to
    autograd with `lam` [M] a constant: grad_o = segment_sum(g, ray_id), grad_d = segment_sum(lam[:, None] * g, ray_id),
    both by dvgo_segment_sum into zero-filled [N,3] (a ray without samples gets exact zeros).  `ray_id` [M] int64 ascending,
    as every sampler here writes it.  rays_o / rays_d [N,3] float32 CUDA tensors."""
    return _RayPoints.apply(rays_o, rays_d, lam, ray_id, pts)


class _ContractPoints(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rays_o, rays_d, ray_id, step_id, q, center, radius, t_tab, bg_len, l2):
        for x, name in ((rays_o, 'rays_o'), (rays_d, 'rays_d'), (q, 'q'), (t_tab, 't_tab')):
            check_input(x, name); check_f32(x, name)
        for x, name in ((ray_id, 'ray_id'), (step_id, 'step_id')):
            check_input(x, name)
            if x.dtype != torch.int64:
                raise RuntimeError(f'{name} must be int64')
        if q.dim() != 2 or q.shape[1] != 3 or ray_id.shape != step_id.shape or ray_id.shape != q.shape[:1]:
            raise RuntimeError('q must be [M,3], ray_id and step_id [M]')
        if rays_o.shape != rays_d.shape or rays_o.dim() != 2 or rays_o.shape[1] != 3:
            raise RuntimeError('rays_o and rays_d must be [N,3]')
        if t_tab.dim() != 1 or t_tab.shape[0] == 0:
            raise RuntimeError('t_tab must be a non-empty vector')
        ctx.save_for_backward(rays_o, rays_d, ray_id, step_id, t_tab)
        ctx.consts = (L.f3(center), L.f3(radius), float(bg_len), int(l2))
        return q.clone()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        rays_o, rays_d, ray_id, step_id, t_tab = ctx.saved_tensors
        center, radius, bg_len, l2 = ctx.consts
        N, dev = rays_o.shape[0], rays_o.device
        g = g.contiguous()
        off = ray_offsets(ray_id, N)
        grad_o = torch.empty((N, 3), dtype=torch.float32, device=dev)       # every row is written by the kernel
        grad_d = torch.empty((N, 3), dtype=torch.float32, device=dev)
        with L.device_of(rays_o):
            L.call('dvgo_contract_ray_bwd', rays_o, rays_d, N, center, radius, t_tab, t_tab.shape[0], bg_len, l2, g, step_id,
                   g.shape[0], off, grad_o, grad_d, stream_of(rays_o))
        return (grad_o if ctx.needs_input_grad[0] else None, grad_d if ctx.needs_input_grad[1] else None, None, None, None,
                None, None, None, None, None)


def contract_points(rays_o, rays_d, ray_id, step_id, q, center, radius, t_tab, bg_len, contracted_norm):
    """The contracted sampler's positions as a differentiable function of their rays: the counterpart of `ray_points` for
    DirectContractedVoxGO.  Returns `q` [M,3] unchanged, bit for bit (what the sampling kernel wrote), and states to autograd
    that row m is the contracted sample of ray ray_id[m] at the table's distance t_tab[step_id[m]]:
        o' = (o - c) / r,  u = d / r,  d' = u / ||u||,  p = o' + d' * t,  q = p if n <= 1 else p * ((1 + b) / n - b / n^2),
        n = max|p_a| ('inf') or ||p||_2 ('l2')
    with `t_tab` a constant.  The backward is csrc/contract_raygrad.hip (dvgo_contract_ray_bwd, include/dvgo_hip.h states the
    arithmetic): the contraction's Jacobian per sample -- at an inf-norm tie the LOWEST axis index attaining max|p_a| carries
    the norm's derivative, and n == 1 exactly is the identity -- summed per ray in a fixed order, then the ray's own Jacobian,
    the normalisation of d included.  A ray without samples gets exact zeros.  Once differentiable.
    `ray_id`, `step_id` [M] int64, ray_id ascending as every sampler here writes it; rays_o / rays_d [N,3] and t_tab [n_max]
    float32 CUDA tensors; `center`, `radius`: 3 floats each (tensor, sequence or host array)."""
    if contracted_norm not in ('inf', 'l2'):
        raise ValueError(f"contracted_norm must be 'inf' or 'l2', got {contracted_norm!r}")
    return _ContractPoints.apply(rays_o, rays_d, ray_id, step_id, q, center, radius, t_tab, bg_len,
                                 1 if contracted_norm == 'l2' else 0)


def total_variation_add_grad(param, grad, wx, wy, wz, dense_mode, x_range=None):
    """total_variation_cuda.total_variation_add_grad (lib/cuda/total_variation.cpp:16-24);
    in place on ``grad``; param/grad [1,C,X,Y,Z] sharing one (dense) stride pattern.
    ``x_range=(lo, hi)``: only the planes lo <= x < hi (the slab a data-parallel rank owns)."""
    if not (param.is_cuda and grad.is_cuda):
        raise RuntimeError('param must be a CUDA tensor')
    if param.stride() != grad.stride():
        raise RuntimeError('param and grad must share strides')
    C, X, Y, Z, sC, sX, sY, sZ = _grid_geom(param)
    lo, hi = (0, X) if x_range is None else x_range
    with L.device_of(param):
        L.call('dvgo_total_variation_add_grad_slab', param, grad, float(wx), float(wy), float(wz), C, X, Y, Z, sC, sX, sY, sZ,
               1 if dense_mode else 0, lo, hi, stream_of(param))


def plane_reg_add_grad(params, grads, weights, dense_mode):
    """Total-variation and L1 regularisers of plane-shaped parameters added to their gradients, in place on ``grads``, in
    ONE launch for the whole list (csrc/plane_tv.hip; include/dvgo_hip.h states the arithmetic).  ``params`` / ``grads``:
    up to 8 float32 tensors [1,C,H,W] (a line is [1,R,N,1]), each gradient sharing its parameter's (dense) strides;
    ``weights``: per tensor (wh, ww, wl1), already normalised -- the kernel divides nothing.  No autograd."""
    n = len(params)
    if len(grads) != n or len(weights) != n:
        raise ValueError(f'plane_reg_add_grad: {n} params, {len(grads)} grads, {len(weights)} weights')
    if n == 0:
        return
    for p, g in zip(params, grads):
        if not (p.is_cuda and g.is_cuda):
            raise RuntimeError('param must be a CUDA tensor')
        check_f32(p, 'param')
        check_f32(g, 'grad')
        if p.dim() != 4 or p.shape[0] != 1 or g.shape != p.shape:
            raise RuntimeError('param and grad must be [1,C,H,W]')
        if p.stride() != g.stride():
            raise RuntimeError('param and grad must share strides')
    table = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])          # noqa: E731  (formed in the call below)
    with L.device_of(params[0]):
        L.call('dvgo_plane_reg_add_grad', table(params), table(grads),
               (ctypes.c_int64 * (3 * n))(*[s for p in params for s in p.shape[1:]]),
               (ctypes.c_int64 * (3 * n))(*[s for p in params for s in p.stride()[1:]]),
               (ctypes.c_float * (3 * n))(*[float(w) for ws in weights for w in ws]),
               n, 1 if dense_mode else 0, stream_of(params[0]))
