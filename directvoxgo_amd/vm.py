"""VMTriPlaneVoxGO: the tri-plane model with TensoRF's vector-matrix (VM) decomposed colour features (Chen et al., ECCV
2022, arXiv:2203.09517), on the MI355X kernels.

The additive tri-plane of TriPlaneVoxGO can only express a sum of three 2-D functions.  Here every one of the `n_comp`
components of a plane is multiplied by a 1-D line along the world axis that plane does not see (xy: x, yz: z, zx: y), and
the 3 * n_comp products are mixed by a basis matrix into the `rgbnet_dim` features the colour head reads:

    features = vm_sample(planes, lines, pts) @ basis            [M, 3 n_comp] @ [3 n_comp, rgbnet_dim]

The sampler and its gradient are one HIP op (ops.vm_sample, csrc/vm.hip; include/dvgo_hip.h states the arithmetic); the
matmul is torch's.  Density stays the dense 3-D grid on the fused march, as in the base.  No equality with any other
implementation is claimed: the contract is INTEGRATION.md section 6d, held by tests/vm_oracle.py.

`raygrad=True` (constructor option, default False; a plain attribute like HashVoxGO.raygrad, not a `get_kwargs` key and not
in checkpoints: pass it to the constructor or to `load_model(VMTriPlaneVoxGO, path, raygrad=True)`): with grad mode on and
`rays_o` or `rays_d` requiring grad, `forward` and `render` take DirectVoxGO._forward_raygrad whatever `self.fused` says --
the sampler's own positions known to autograd as o + d * lam (ops.ray_points), the density through the
position-differentiable trilinear op, the features through `vm_sample(..., position_grad=True) @ basis` (csrc/vm_xyz.hip),
the per-ray sum the model's in-order one -- so that pose.refine_poses can move the cameras.  The stop-gradients are
`_forward_raygrad`'s (lam constant, the kept set fixed, no gradient for viewdirs), and every key of the result has the bits
of the `fused=False` forward on the same detached rays.  Rays that do not require grad, and every path of a model without
the option, are untouched by it.

`raygrad='fused'` sets `raygrad` and, on the instance, `fused_raygrad` (no `get_kwargs` key either, not in checkpoints:
`load_model(VMTriPlaneVoxGO, path, raygrad='fused')`): with `self.fused`, rays that require grad stay on the fused march --
`fused_march(positions=True, raygrad=True)`, whose backward launches dvgo_march_ray_bwd_pts (csrc/march_raygrad.hip)
first: the density's share of every record plus what `vm_sample(..., position_grad=True)` returned for the positions, summed
per ray -- with the fused forward's bits in every key and the same stop-gradients; `viewdirs` is detached.  With
`fused=False` such rays take `_forward_raygrad` as before.  `pose.refine_poses(fused=True)` accepts the model only with it.

Everything the base leaves out stays out: extract_mesh, data-parallel training, pose refinement without `raygrad=True`, the
plane decoders' options and the encoder's keys.  Not built either: the basis matmul fused into the sampler.  (The VM-decomposed density is
tensorf.TensoRFVoxGO.)

Regularisers (TensoRF trains its VM model with them): `plane_regularizers_add_grad` adds total variation on the planes,
total variation on the lines and L1 on the lines to the six gradients in one HIP launch (ops.plane_reg_add_grad,
csrc/plane_tv.hip).  TrainStep reads `weight_tv_planes`, `weight_tv_lines` and `weight_l1_lines`
from the config (absent: 0, nothing runs) inside the usual tv_after / tv_before / tv_every window.  VM_FINE_TRAIN sets none
of them: no weight has been tuned on this model.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .ops import PLANE_KEYS, vm_sample
from .triplane import TRI_FINE_TRAIN, TriPlaneVoxGO
from .voxel_model import _rays_want_grad

# which world axis the line of each plane follows: the one the plane's rows and columns do not
LINE_AXIS = {'xy': 0, 'yz': 2, 'zx': 1}

# TRI_FINE_TRAIN with TensoRF's published rates: 2e-2 for the grids (planes and lines), 1e-3 for the networks (the basis).
# They are the paper's numbers and have not been tuned on this model.
VM_FINE_TRAIN = dict(TRI_FINE_TRAIN, lrate_planes=2e-2, lrate_lines=2e-2, lrate_basis=1e-3)


class VMTriPlaneVoxGO(TriPlaneVoxGO):
    """TriPlaneVoxGO whose colour features are `vm_sample(planes, lines, pts) @ basis`.  Takes the base's arguments plus
    `n_comp` (components per plane, R) and `line_size` (an int: the length of all three lines; None: each line takes the
    `world_size` extent of its axis and is resized with the grid).  `rgbnet_dim` is the feature width the head sees.
    `tri_aggregation` is not an option: the products are concatenated in front of the basis.  `raygrad`: rays that require
    grad are differentiated (module docstring)."""

    def __init__(self, xyz_min, xyz_max, n_comp=16, line_size=None, raygrad=False, **kwargs):
        if kwargs.pop('tri_aggregation', 'concat') != 'concat':
            raise ValueError("tri_aggregation is not an option of VMTriPlaneVoxGO: the 3 * n_comp products are concatenated "
                             "and mixed by `basis`")
        if int(n_comp) < 1:
            raise ValueError(f'n_comp must be at least 1, got {n_comp}')
        if line_size is not None and int(line_size) < 1:
            raise ValueError(f'line_size must be at least 1, got {line_size}')
        object.__setattr__(self, 'n_comp', int(n_comp))          # read by _alloc_plane, which the base constructor calls
        # rays that require grad are differentiated; not in get_kwargs (module docstring).  Set ahead of the base constructor,
        # whose occupancy mask may already sample the model
        object.__setattr__(self, 'raygrad', bool(raygrad))
        if raygrad == 'fused':               # ... on the fused march where there is one (DirectVoxGO.fused_raygrad, per instance)
            object.__setattr__(self, 'fused_raygrad', True)
        super().__init__(xyz_min, xyz_max, **kwargs)
        self.line_size = None if line_size is None else int(line_size)
        self.lines = nn.ParameterDict({k: nn.Parameter(self._alloc_line(self._line_n(k))) for k in PLANE_KEYS})
        self.basis = nn.Parameter(nn.Linear(3 * self.n_comp, self.rgbnet_dim, bias=False).weight.detach().t().contiguous())

    # ------------------------------------------------------------------ construction
    def _feature_width(self):
        return self.rgbnet_dim               # what `basis` emits

    def _alloc_plane(self, hw, device=None):
        # a product of two zero tensors has a zero gradient for ever: TensoRF's 0.1 * randn, from torch's global generator
        p = 0.1 * torch.randn([1, self.n_comp, *hw], device=device)
        return p.contiguous(memory_format=torch.channels_last) if self.channels_last else p

    def _line_n(self, key):
        """The length of line `key`: `line_size`, else the world_size extent of the axis it follows."""
        return self.line_size if self.line_size is not None else int(self.world_size[LINE_AXIS[key]])

    def _alloc_line(self, n, device=None):
        ln = 0.1 * torch.randn([1, self.n_comp, n, 1], device=device)
        return ln.contiguous(memory_format=torch.channels_last) if self.channels_last else ln

    def get_kwargs(self):
        kw = super().get_kwargs()
        del kw['tri_aggregation']
        kw.update(n_comp=self.n_comp, line_size=self.line_size)
        return kw

    # ------------------------------------------------------------------ grid maintenance
    @torch.no_grad()
    def scale_volume_grid(self, num_voxels):
        """The base's (density, occupancy, planes), plus the lines: resized with the grid, bilinear with
        align_corners=True on [1, R, N, 1], when they take their lengths from world_size; left alone under `line_size`."""
        super().scale_volume_grid(num_voxels)
        if self.line_size is None:
            for k in PLANE_KEYS:
                ln = F.interpolate(self.lines[k].data.contiguous(), size=(self._line_n(k), 1), mode='bilinear', align_corners=True)
                if self.channels_last:
                    ln = ln.contiguous(memory_format=torch.channels_last)
                self.lines[k] = nn.Parameter(ln)

    def _plane_reg_items(self, weight_tv_planes, weight_tv_lines, weight_l1_lines):
        """What `plane_regularizers_add_grad` (the base's) hands to its single launch: the base's planes, then the three
        lines with total variation along each (wh = weight_tv_lines * N / 128 / 2: a node has 2 neighbours) and L1
        (wl1 = weight_l1_lines: weight * sgn(value), not scaled by resolution)."""
        items = super()._plane_reg_items(weight_tv_planes, 0.0, 0.0)
        if weight_tv_lines != 0 or weight_l1_lines != 0:
            for k in PLANE_KEYS:
                ln = self.lines[k]
                w = weight_tv_lines * ln.shape[2] / 128 / 2
                items.append((ln, (w, 0.0, weight_l1_lines)))
        return items

    # ------------------------------------------------------------------ forward
    def render(self, feats, rays_o, rays_d, viewdirs, global_step=None, **render_kwargs):
        """The base's `render`; with `raygrad=True`, rays that require grad take DirectVoxGO._forward_raygrad on the same
        `feats` (the module docstring says what that means) or, with `raygrad='fused'` on a fused model, the base's fused
        render with the march's own ray backward."""
        if self.raygrad and _rays_want_grad(rays_o, rays_d) and not (self.fused_raygrad and self.fused):
            return self._forward_raygrad(rays_o, rays_d, viewdirs, feats=feats, **render_kwargs)
        return super().render(feats, rays_o, rays_d, viewdirs, global_step, **render_kwargs)

    # ------------------------------------------------------------------ features
    def sample_planes(self, pts, feats=None):
        """[M, rgbnet_dim].  `feats`: the planes under 'xy', 'yz', 'zx' and, optionally, lines under 'xy_line', 'yz_line',
        'zx_line'; a missing line key means the model's own line.  The basis is always the model's.  With `raygrad=True`,
        positions that require grad receive theirs."""
        planes = self.planes if feats is None else feats
        lines = {k: planes[k + '_line'] if k + '_line' in planes else self.lines[k] for k in PLANE_KEYS}
        return vm_sample(planes, lines, pts, self.xyz_min, self.xyz_max, position_grad=self.raygrad) @ self.basis
