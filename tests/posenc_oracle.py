"""Float64 statement of the positional-encoding colour head (test infrastructure): forward and the six weight / bias
gradients of directvoxgo_amd.shade.shade_posenc (lib/dvgo.py:528-534), with a magnitude for every output.

    x   = cat([p, sin(p (x) freq), cos(p (x) freq), emb[ray_id]])       p = the float32 sample positions
    rgb = sigmoid(relu(relu(x W1^T + b1) W2^T + b2) W3^T + b3)           no diffuse term

Once x is formed this is the direct form of the feature-grid head, so the chain, magnitudes and gradients are
tests/shade_oracle.py's, evaluated with x in place of cat([feat, emb[ray_id]]).  `rows` hands out that chain's per-row
intermediates (h1, h2, gz, G1, the ReLU decisions) for the arrays the kernels store (tests/test_gpu_posenc_oracle.py).

The position features.  The argument p * 2^j is exact in float32 (scaling by a power of two), so the kernel's sinf /
cosf and the float64 sin / cos here see the same argument; the kernel's result is within a few ulp of its own value
(sinf / cosf are the full-range library functions, not the hardware approximation).  Each such x_k therefore carries an
error of a few u |x_k|, which enters z1 as at most a few u * (|x| |W1|^T) = a few u * A1: a few more terms of the
layer-1 chain, nothing more.

Bounds: shade_oracle's K_ROW = 1024 and K_SUM = 2048, argued again for this head.
  K_ROW: the layer-1 chain has d_in + 1 <= 97 terms, layers 2 and 3 have 129 each: n <= 355, plus <= 4 u for the
         position features above and a few ulp for expf and the division of the sigmoid.  The backward chain
         (3 + 128 + 128) sits on top of the forward error carried in through rgb.  All of it is < 700 < 2^10.
  K_SUM: the weight gradients are sums over M rows of per-row terms that each obey K_ROW.  The kernel (pe_wgrad_kernel)
         sums ceil(M / 32 / n_parts) 32-row tiles per workgroup in one MFMA chain (n_parts <= 512), then the 512 partials
         in 16 slices of <= 32 (four interleaved accumulators) met by atomics.  With M <= 2^22 a chain has at most
         8192 + 512 terms, and the probabilistic bound lambda sqrt(n) u of Higham & Mary (2019) stays below
         6 * 93 = 558.  2^10 + 558 is rounded up to 2^11.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shade_oracle as S  # noqa: E402

U, K_ROW, K_SUM = S.U, S.K_ROW, S.K_SUM
params_of, excess, assert_close, split_ties = S.params_of, S.excess, S.assert_close, S.split_ties
SUM_KEYS = S.SUM_KEYS


def pos_embed(pts, freq):
    """cat([p, sin(p (x) freq), cos(p (x) freq)]) in float64 from the float32 argument (exact: freq holds powers of two),
    flattened component-major as (pts.unsqueeze(-1) * posfreq).flatten(-2) is."""
    p = pts.float()
    arg = (p.unsqueeze(-1) * freq.float().to(p.device)).flatten(-2).double()
    return torch.cat([p.double(), arg.sin(), arg.cos()], -1)


def view_embed(viewdirs, viewfreq):
    """Per-ray view embedding in float64 from the same float32 arguments (lib/dvgo.py:524-525)."""
    return pos_embed(viewdirs, viewfreq)


def forward(P, pts, freq, emb, ray_id):
    """rgb, its magnitude and the per-row ReLU margin (float64).  `emb` is the per-ray view embedding as the kernel
    reads it (the float32 output of viewdir_embed)."""
    return S.forward(P, pos_embed(pts, freq), emb, ray_id, diffuse=False)


ROW_KEYS = ('rgb', 'h1', 'h2', 'gz', 'G1')


def rows(P, pts, freq, emb, ray_id, g_rgb):
    """The per-row quantities the kernels store, float64: dict of values and dict of magnitudes for rgb, h1, h2
    (magnitudes A1m, A2m), gz (Bgz) and G1 (B1), all bound K_ROW: each is a prefix of the chain K_ROW was argued for.
    The values dict also holds the ReLU decisions k1, k2 [M,width] (bool) and 'margin' [M].  These are the intermediates
    of shade_oracle's chain, not a second statement of it."""
    out = {k: [] for k in ROW_KEYS + ('k1', 'k2', 'margin')}
    mags = {k: [] for k in ROW_KEYS}
    x = pos_embed(pts, freq)
    with torch.no_grad():
        for s in range(0, x.shape[0], S.CHUNK):
            sl = slice(s, s + S.CHUNK)
            st = S._rows(P, x[sl], emb, ray_id[sl], False)
            gz, Bgz, _, _, G1, B1 = S._back_rows(P, st, g_rgb[sl])
            margin = torch.minimum(S._relu_margin(st['z1'], st['A1']), S._relu_margin(st['z2'], st['A2']))
            for k, v, m in (('rgb', st['rgb'], st['rgb_mag']), ('h1', st['h1'], st['A1m']), ('h2', st['h2'], st['A2m']),
                            ('gz', gz, Bgz), ('G1', G1, B1)):
                out[k].append(v)
                mags[k].append(m)
            for k, v in (('k1', st['k1']), ('k2', st['k2']), ('margin', margin)):
                out[k].append(v)
    width = P[0].shape[0]
    empty = dict(rgb=(0, 3), gz=(0, 3), margin=(0,))

    def cat(k, parts, dtype=torch.float64):
        return torch.cat(parts) if parts else torch.empty(empty.get(k, (0, width)), dtype=dtype, device=x.device)
    return ({k: cat(k, v, torch.bool if k in ('k1', 'k2') else torch.float64) for k, v in out.items()},
            {k: cat(k, v) for k, v in mags.items()})


def forward_backward(P, pts, freq, emb, ray_id, g_rgb):
    """dict of values and dict of magnitudes: rgb [M,3] (bound K_ROW); gW1 gb1 gW2 gb2 gW3 gb3 (bound K_SUM); margin."""
    out, mags = S.forward_backward(P, pos_embed(pts, freq), emb, ray_id, g_rgb, diffuse=False)
    del out['g_feat'], mags['g_feat']          # positions carry no gradient
    return out, mags
