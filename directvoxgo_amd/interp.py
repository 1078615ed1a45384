"""InterpTriPlaneVoxGO: the reference fork's tri-plane model with its bilinear plane decoder (lib/tri_dvgo.py, the
`implicit_voxel_feat=True, liif=False` path its two multi-scene configs set), on the MI355X kernels.

Where LIIFTriPlaneVoxGO decodes the nearest texel at four shifted positions, this model decodes one row per sample and
plane (lib/tri_dvgo.py:568-607 interpolate): the plane's bilinear features, the bilinear sample (q0, q1) of a coordinate
table laid over the world lattice, sin / cos of q * 2^j for the `posbase_pe` frequencies and, with `cell_decode`, two cell
sizes go through an MLP (`liif.InterpMLP`); the three predictions are concatenated or summed.  The rows and the gradient of
their feature columns are HIP (ops.plane_rows, csrc/plane_rows.hip); the MLPs are torch modules, run in two batches
(`ops.interp_decode`).

Mirrored from the reference as it stands:
  * plane zx is decoded by `interp_yz`; `interp_zx` exists, is in the state_dict and never receives a gradient;
  * the coordinate table of a plane follows the world lattice of the plane's name and is addressed by the flipped
    coordinates; its extents follow `world_size`, whatever the planes' sizes;
  * the cell sizes are 1 / world_size extents, not scaled by the plane size;
  * `posbase_pe=0` cannot run there (interpolate reads a `posfreq` buffer that was never registered): a ValueError here.
`cat_posemb=True` appends the positions' own encoding to the decoded features (lib/tri_dvgo.py:772-775).
"""
import torch

from .liif import InterpMLP
from .ops import interp_decode
from .triplane import TRI_FINE_TRAIN, TriPlaneVoxGO
from .voxel_model import _freqs, _posenc

# configs/nerf/tri_multiscene.py's fine stage without the encoder / mapping groups; the planes keep TRI_FINE_TRAIN's rate
# (the reference trains the encoder that emits them)
TRI_INTERP_FINE_TRAIN = dict(TRI_FINE_TRAIN, N_iters=50000, N_rand=4096, lrate_interp_xy=5e-4, lrate_interp_yz=5e-4,
                             lrate_interp_zx=5e-4, lrate_rgbnet=1e-3, lrate_decay=1000, pg_scale=[1000, 2000, 3000, 5000],
                             weight_entropy_last=0.001, weight_rgbper=0)

_LEFT_OUT = {
    'feat_unfold': 'the 3x3 feature unfolding in front of the decoder is not built',
    'no_voxel_feat': 'a colour head that reads the positional embedding instead of the plane features is not built',
}


class InterpTriPlaneVoxGO(TriPlaneVoxGO):
    """TriPlaneVoxGO whose colour features are `interp_decode(planes, {interp_xy, interp_yz}, pts)`.  Takes the
    reference's options `implicit_voxel_feat=True` and `liif=False` (both implied), `cell_decode`, `interp_width`,
    `interp_depth`, `posbase_pe` (at least 1; it defaults to the reference's 0, which raises) and `cat_posemb`;
    `interp_dropout` is Interp_MLP's `dropout`; `local_ensemble` is accepted and ignored, as the reference reads it in the LIIF path only."""

    def __init__(self, xyz_min, xyz_max, **kwargs):
        if not kwargs.pop('implicit_voxel_feat', True):
            raise NotImplementedError('implicit_voxel_feat=False is the bilinear path without a decoder: use triplane.TriPlaneVoxGO')
        if kwargs.pop('liif', False):
            raise NotImplementedError('liif=True is the LIIF plane decoder: use liif.LIIFTriPlaneVoxGO')
        for key, why in _LEFT_OUT.items():
            if kwargs.pop(key, False):
                raise NotImplementedError(f'{key}: {why}')
        kwargs.pop('local_ensemble', None)
        opts = dict(cell_decode=bool(kwargs.pop('cell_decode', True)), interp_width=int(kwargs.pop('interp_width', 64)),
                    interp_depth=int(kwargs.pop('interp_depth', 2)), interp_dropout=float(kwargs.pop('interp_dropout', 0.1)),
                    posbase_pe=int(kwargs.pop('posbase_pe', 0)), cat_posemb=bool(kwargs.pop('cat_posemb', False)))
        if opts['posbase_pe'] < 1:
            raise ValueError('posbase_pe must be given and at least 1 (the default is the reference\'s, 0): the reference\'s own '
                             'interpolate reads a `posfreq` buffer that it registers only for posbase_pe > 0 '
                             '(lib/tri_dvgo.py:208-209, :590)')
        if opts['interp_depth'] < 2:
            raise ValueError('interp_depth must be at least 2')
        object.__setattr__(self, '_interp_opts', opts)          # read by _init_head, which the base constructor calls
        super().__init__(xyz_min, xyz_max, **kwargs)
        self.cell_decode, self.posbase_pe, self.cat_posemb = opts['cell_decode'], opts['posbase_pe'], opts['cat_posemb']
        self.register_buffer('posfreq', _freqs(self.posbase_pe))
        dim0 = self.rgbnet_dim + 2 + 4 * self.posbase_pe + (2 if self.cell_decode else 0)          # lib/tri_dvgo.py:154-165
        for key in ('interp_xy', 'interp_yz', 'interp_zx'):
            setattr(self, key, InterpMLP(dim0, self.rgbnet_dim, opts['interp_width'], opts['interp_depth'], opts['interp_dropout']))

    def _init_head(self, mlp_feat_dim, viewbase_pe, rgbnet_width, rgbnet_depth):
        o = self._interp_opts
        pos = (3 + 3 * o['posbase_pe'] * 2) if o['cat_posemb'] else 0      # lib/tri_dvgo.py:215-216
        super()._init_head(mlp_feat_dim + pos, viewbase_pe, rgbnet_width, rgbnet_depth)

    def get_kwargs(self):
        kw = super().get_kwargs()
        kw.update(implicit_voxel_feat=True, liif=False, feat_unfold=False, **self._interp_opts)
        return kw

    def sample_planes(self, pts, feats=None):
        """interpolate (lib/tri_dvgo.py:568-607) at the current world_size: [M, 3 * rgbnet_dim] or, 'sum',
        [M, rgbnet_dim].  Dropout follows `self.training`."""
        return interp_decode(self.planes if feats is None else feats, {'xy': self.interp_xy, 'yz': self.interp_yz}, pts,
                             self.xyz_min, self.xyz_max, [int(v) for v in self.world_size], self.posbase_pe, self.cell_decode,
                             self.tri_aggregation)

    def _head_features(self, pts, feats):
        k0 = self.sample_planes(pts, feats)
        if self.cat_posemb:                                  # lib/tri_dvgo.py:772-775: [k0_view, pos_emb, viewdirs_emb]
            k0 = torch.cat([k0, _posenc(pts, self.posfreq)], -1)
        return k0
