"""LIIFTriPlaneVoxGO: the reference fork's tri-plane model with its LIIF plane decoder (lib/tri_dvgo.py, the
`implicit_voxel_feat=True, liif=True` path every one of its tri-plane configs sets), on the MI355X kernels.

Where TriPlaneVoxGO reads a sample's colour features bilinearly off the three planes, this model decodes them
(lib/tri_dvgo.py:481-565 liif_interpolate): per plane and per shifted position (four with `local_ensemble`, else one) the
nearest texel's features, two relative coordinates and, with `cell_decode`, two cell sizes go through an MLP
(`InterpMLP` = lib/mlp.py:88-101 Interp_MLP), and the predictions are blended by the opposite corner's area.  The rows,
the weights, the blend and their gradients are HIP (ops.liif_gather / liif_blend, csrc/liif.hip); the MLPs are torch
modules, run in two batches (`ops.liif_decode`).

Mirrored from the reference as it stands:
  * plane zx is decoded by `interp_yz`; `interp_zx` exists, is in the state_dict and never receives a gradient;
  * the first relative coordinate is taken against the column table and the second against the row table;
  * the coordinate table follows `world_size`, whatever the planes' sizes.
`posbase_pe=P` with `cat_posemb=True` appends the positions' encoding to the decoded features (lib/tri_dvgo.py:772-775).
"""
import torch
import torch.nn as nn

from .ops import liif_decode
from .triplane import TRI_FINE_TRAIN, TriPlaneVoxGO
from .voxel_model import _freqs, _posenc, mlp_forward

# configs/nerf/tri_lego.py's fine stage; the planes keep TRI_FINE_TRAIN's rate (the reference trains the encoder that emits them)
TRI_LIIF_FINE_TRAIN = dict(TRI_FINE_TRAIN, N_iters=200000, N_rand=4096, lrate_interp_xy=5e-4, lrate_interp_yz=5e-4,
                           lrate_interp_zx=5e-4, lrate_rgbnet=5e-4, lrate_decay=400, pg_scale=[5000, 8000, 12000, 15000])


class InterpMLP(nn.Module):
    """lib/mlp.py:88-101 Interp_MLP, same module tree (state_dict keys model.0, model.{2..depth-1}.0, model.{depth})."""

    def __init__(self, in_dim, out_dim, width=128, depth=5, dropout=0.1):
        super().__init__()
        self.model = nn.Sequential(
            nn.Linear(in_dim, width), nn.ReLU(inplace=True),
            *[nn.Sequential(nn.Linear(width, width), nn.Dropout(p=dropout), nn.ReLU(inplace=True)) for _ in range(depth - 2)],
            nn.Linear(width, out_dim))

    def forward(self, x):
        return mlp_forward(self.model, x)


_LEFT_OUT = {
    'feat_unfold': 'the 3x3 feature unfolding in front of the decoder is not built',
    'no_voxel_feat': 'a colour head that reads the positional embedding instead of the plane features is not built',
}


class LIIFTriPlaneVoxGO(TriPlaneVoxGO):
    """TriPlaneVoxGO whose colour features are `liif_decode(planes, {interp_xy, interp_yz}, pts)`.  Takes the
    reference's options `implicit_voxel_feat` and `liif` (both implied), `cell_decode`, `local_ensemble`, `interp_width`,
    `interp_depth`, and `posbase_pe` with `cat_posemb`; `interp_dropout` is Interp_MLP's `dropout`."""

    def __init__(self, xyz_min, xyz_max, **kwargs):
        if not kwargs.pop('implicit_voxel_feat', True):
            raise NotImplementedError('implicit_voxel_feat=False is the bilinear path: use triplane.TriPlaneVoxGO')
        if not kwargs.pop('liif', True):
            raise NotImplementedError('liif=False with implicit_voxel_feat=True (the bilinear `interpolate` decoder, '
                                      'lib/tri_dvgo.py:568-607) is interp.InterpTriPlaneVoxGO')
        for key, why in _LEFT_OUT.items():
            if kwargs.pop(key, False):
                raise NotImplementedError(f'{key}: {why}')
        opts = dict(cell_decode=bool(kwargs.pop('cell_decode', True)), local_ensemble=bool(kwargs.pop('local_ensemble', True)),
                    interp_width=int(kwargs.pop('interp_width', 64)), interp_depth=int(kwargs.pop('interp_depth', 2)),
                    interp_dropout=float(kwargs.pop('interp_dropout', 0.1)), posbase_pe=int(kwargs.pop('posbase_pe', 0)),
                    cat_posemb=bool(kwargs.pop('cat_posemb', False)))
        if opts['interp_depth'] < 2:
            raise ValueError('interp_depth must be at least 2')
        object.__setattr__(self, '_liif_opts', opts)          # read by _init_head, which the base constructor calls
        super().__init__(xyz_min, xyz_max, **kwargs)
        self.cell_decode, self.local_ensemble = opts['cell_decode'], opts['local_ensemble']
        self.posbase_pe, self.cat_posemb = opts['posbase_pe'], opts['cat_posemb']
        if self.posbase_pe > 0:
            self.register_buffer('posfreq', _freqs(self.posbase_pe))
        dim0 = self.rgbnet_dim + 2 + (2 if self.cell_decode else 0)          # lib/tri_dvgo.py:154-165
        for key in ('interp_xy', 'interp_yz', 'interp_zx'):
            setattr(self, key, InterpMLP(dim0, self.rgbnet_dim, opts['interp_width'], opts['interp_depth'], opts['interp_dropout']))

    def _init_head(self, mlp_feat_dim, viewbase_pe, rgbnet_width, rgbnet_depth):
        o = self._liif_opts
        pos = (3 + 3 * o['posbase_pe'] * 2) if (o['posbase_pe'] > 0 and o['cat_posemb']) else 0      # lib/tri_dvgo.py:215-216
        super()._init_head(mlp_feat_dim + pos, viewbase_pe, rgbnet_width, rgbnet_depth)

    def get_kwargs(self):
        kw = super().get_kwargs()
        kw.update(implicit_voxel_feat=True, liif=True, feat_unfold=False, **self._liif_opts)
        return kw

    def sample_planes(self, pts, feats=None):
        """liif_interpolate (lib/tri_dvgo.py:481-565) at the current world_size: [M, 3 * rgbnet_dim] or, 'sum',
        [M, rgbnet_dim].  Dropout follows `self.training`."""
        return liif_decode(self.planes if feats is None else feats, {'xy': self.interp_xy, 'yz': self.interp_yz}, pts,
                           self.xyz_min, self.xyz_max, [int(v) for v in self.world_size], self.cell_decode, self.local_ensemble,
                           self.tri_aggregation)

    def _head_features(self, pts, feats):
        k0 = self.sample_planes(pts, feats)
        if self.posbase_pe > 0 and self.cat_posemb:          # lib/tri_dvgo.py:772-775: [k0_view, pos_emb, viewdirs_emb]
            k0 = torch.cat([k0, _posenc(pts, self.posfreq)], -1)
        return k0
