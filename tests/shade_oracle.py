"""Float64 statement of the colour head (test infrastructure): forward, ReLU decisions, data gradient and the six weight /
bias gradients of directvoxgo_amd.shade.shade, for the diffuse and the direct form (lib/dvgo.py:516-541), with a
magnitude for every output.

    x   = cat([feat[:, 3:] if diffuse else feat, emb[ray_id]])
    z1  = x W1^T + b1,   h1 = relu(z1)
    z2  = h1 W2^T + b2,  h2 = relu(z2)
    z3  = h2 W3^T + b3 (+ feat[:, :3] if diffuse),  rgb = sigmoid(z3)
    gz  = g * rgb (1 - rgb),  G2 = [z2 > 0] (gz W3),  G1 = [z1 > 0] (G2 W2),  gx = G1 W1
    g_feat = gx[:, :n_view] (diffuse: [gz, gx[:, :n_view]]),  gW3 = gz^T h2,  gW2 = G2^T h1,  gW1 = G1^T x,  gb* = sums

Magnitudes.  Every quantity above is a chain of dot products.  Its magnitude is the same chain evaluated on absolute
values: A1 = |x||W1|^T + |b1|, A2 = (A1 [z1 > 0]) |W2|^T + |b2|, A3 likewise (+ |feat[:, :3]|), and backwards from
Bgz = |g| (rgb (1 - rgb) A3 + rgb + TINY) + |gz| (TINY: sigmoid underflow, see below).  Whatever order a float32
kernel sums in, its error on a value is at most gamma_n * magnitude, n being the total length of the chain (Higham,
Accuracy and Stability, section 3.1), as long as it takes every ReLU the same way as the exact evaluation.
`render_oracle.relu_margin` is the model.

Bounds are K * 2^-24 * magnitude with two fixed K:
  K_ROW = 1024 for per-row outputs (rgb, g_feat) and ReLU ties.  The forward chain has n <= (40 + 1) + (128 + 1) +
          (128 + 1) = 299 terms.  The bf16 3-way split (csrc/shade_x3.hip) drops products below 2^-23 |x w|, which adds
          at most 2 per layer.  expf and the division of the sigmoid add a few ulp.  The backward chain (3 + 128 + 128
          terms) sits on top of the forward error carried in through rgb.  All of it is < 600, rounded up to 2^10.
  K_SUM = 2048 for the weight and bias gradients.  Each of them is a sum over the M rows of per-row terms that each obey
          K_ROW.  The row sums are blocked: at most ceil(M / 512) rows per partial, then 512 partials.  A worst-case
          bound would grow with M, so this uses the probabilistic bound lambda sqrt(n) u of Higham & Mary (2019): with
          n <= 8192 + 512 it stays below 6 * 93 = 558.  2^10 + 558 is rounded up to 2^11.
A subtly wrong kernel is far outside both.  Dropping one of the six bf16 partial products costs about 2^-9 of the
product, i.e. 2^15 u.  A ReLU mask that passes a dead unit's gradient costs a whole term.

Ties.  A row whose smallest relative ReLU margin |z| / A is below K_ROW u may legitimately take the other branch in
float32.  `split_ties` drops such rows before a batch goes to the kernel.  A unit whose magnitude is exactly zero has
every term zero, so every summation order gives a zero pre-activation.  Its margin is infinite, not zero.
"""
import torch

U = 2.0 ** -24
K_ROW = 1024
K_SUM = 2048
# sigmoid below FLT_MIN: 1 / (1 + expf(-z)) underflows to 0 (expf(-z) = inf for z < -88.7) where the exact value is a
# subnormal.  That absolute error, <= 2^-126, enters rgb's magnitude as TINY (K_ROW u TINY = 2^-126) and from there gz and
# everything downstream.
TINY = 2.0 ** -126 / (K_ROW * U)
CHUNK = 1 << 18          # rows per pass (bounds the float64 temporaries at 4 M rows x 128 features)


def _params(W1, b1, W2, b2, W3, b3, device):
    return [t.detach().to(device=device, dtype=torch.float64) for t in (W1, b1, W2, b2, W3, b3)]


def params_of(rgbnet, device=None):
    """(W1, b1, W2, b2, W3, b3) of a make_rgbnet(d_in, width, 3) module tree, float64."""
    l1, l2, l3 = rgbnet[0], rgbnet[2][0], rgbnet[3]
    device = device if device is not None else l1.weight.device
    return _params(l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias, device)


def _inputs(feat, emb, ray_id, diffuse):
    f = feat.double()
    return torch.cat([f[:, 3:] if diffuse else f, emb.double()[ray_id]], -1)


def _relu_margin(z, A):
    # |z| / A per unit; A == 0 means every term is zero: no tie whatever the order
    m = z.abs() / A.clamp_min(1e-300)
    return torch.where(A == 0, torch.full_like(m, float('inf')), m).amin(1)


def forward(P, feat, emb, ray_id, diffuse):
    """rgb, its magnitude, and the per-row ReLU margin (float64, on feat's device)."""
    W1, b1, W2, b2, W3, b3 = P
    M = feat.shape[0]
    dev = feat.device
    rgb = torch.empty((M, 3), dtype=torch.float64, device=dev)
    mag = torch.empty_like(rgb)
    margin = torch.empty(M, dtype=torch.float64, device=dev)
    with torch.no_grad():
        for s in range(0, M, CHUNK):
            sl = slice(s, s + CHUNK)
            st = _rows(P, feat[sl], emb, ray_id[sl], diffuse)
            rgb[sl], mag[sl] = st['rgb'], st['rgb_mag']
            margin[sl] = torch.minimum(_relu_margin(st['z1'], st['A1']), _relu_margin(st['z2'], st['A2']))
    return rgb, mag, margin


def _rows(P, feat, emb, ray_id, diffuse):
    W1, b1, W2, b2, W3, b3 = P
    x = _inputs(feat, emb, ray_id, diffuse)
    z1 = torch.addmm(b1, x, W1.t())
    A1 = torch.addmm(b1.abs(), x.abs(), W1.abs().t())
    k1 = z1 > 0
    h1, A1m = torch.where(k1, z1, 0.0), torch.where(k1, A1, 0.0)
    z2 = torch.addmm(b2, h1, W2.t())
    A2 = torch.addmm(b2.abs(), A1m, W2.abs().t())
    k2 = z2 > 0
    h2, A2m = torch.where(k2, z2, 0.0), torch.where(k2, A2, 0.0)
    z3 = torch.addmm(b3, h2, W3.t())
    A3 = torch.addmm(b3.abs(), A2m, W3.abs().t())
    if diffuse:
        z3 = z3 + feat[:, :3].double()
        A3 = A3 + feat[:, :3].double().abs()
    rgb = torch.sigmoid(z3)
    ds = rgb * (1 - rgb)
    return dict(x=x, z1=z1, A1=A1, k1=k1, h1=h1, A1m=A1m, z2=z2, A2=A2, k2=k2, h2=h2, A2m=A2m, rgb=rgb, ds=ds,
                rgb_mag=ds * A3 + rgb + TINY)


def _back_rows(P, st, g_rgb):
    """The data gradients of the rows of `st` (= _rows(...)) down to layer 1, value and magnitude:
    gz, Bgz [M,3]; G2, B2 and G1, B1 [M,width]."""
    W1, b1, W2, b2, W3, b3 = P
    g = g_rgb.double()
    gz = g * st['ds']
    Bgz = g.abs() * st['rgb_mag'] + gz.abs()
    G2 = torch.where(st['k2'], gz @ W3, 0.0)
    B2 = torch.where(st['k2'], Bgz @ W3.abs(), 0.0)
    G1 = torch.where(st['k1'], G2 @ W2, 0.0)
    B1 = torch.where(st['k1'], B2 @ W2.abs(), 0.0)
    return gz, Bgz, G2, B2, G1, B1


def forward_backward(P, feat, emb, ray_id, g_rgb, diffuse):
    """Everything, float64 on feat's device: dict of value / magnitude pairs
      rgb, g_feat: [M, 3], [M, C] (per row, bound K_ROW);  gW1 gb1 gW2 gb2 gW3 gb3 (batch sums, bound K_SUM);
    plus 'margin' [M] (smallest relative ReLU margin of the row)."""
    W1, b1, W2, b2, W3, b3 = P
    M, C = feat.shape
    dev = feat.device
    n_view = C - (3 if diffuse else 0)
    out = {'rgb': torch.empty((M, 3), dtype=torch.float64, device=dev),
           'g_feat': torch.empty((M, C), dtype=torch.float64, device=dev),
           'margin': torch.empty(M, dtype=torch.float64, device=dev)}
    mags = {'rgb': torch.empty_like(out['rgb']), 'g_feat': torch.empty_like(out['g_feat'])}
    for k, p in zip(('gW1', 'gb1', 'gW2', 'gb2', 'gW3', 'gb3'), P):
        out[k], mags[k] = torch.zeros_like(p), torch.zeros_like(p)
    with torch.no_grad():
        for s in range(0, M, CHUNK):
            sl = slice(s, s + CHUNK)
            st = _rows(P, feat[sl], emb, ray_id[sl], diffuse)
            out['rgb'][sl], mags['rgb'][sl] = st['rgb'], st['rgb_mag']
            out['margin'][sl] = torch.minimum(_relu_margin(st['z1'], st['A1']), _relu_margin(st['z2'], st['A2']))
            gz, Bgz, G2, B2, G1, B1 = _back_rows(P, st, g_rgb[sl])
            gx, Bx = G1 @ W1, B1 @ W1.abs()
            if diffuse:
                out['g_feat'][sl] = torch.cat([gz, gx[:, :n_view]], 1)
                mags['g_feat'][sl] = torch.cat([Bgz, Bx[:, :n_view]], 1)
            else:
                out['g_feat'][sl], mags['g_feat'][sl] = gx[:, :n_view], Bx[:, :n_view]
            for k, a, b, ma, mb in (('gW3', gz, st['h2'], Bgz, st['A2m']), ('gW2', G2, st['h1'], B2, st['A1m']),
                                    ('gW1', G1, st['x'], B1, st['x'].abs())):
                out[k] += a.t() @ b
                mags[k] += ma.t() @ mb
            for k, a, ma in (('gb3', gz, Bgz), ('gb2', G2, B2), ('gb1', G1, B1)):
                out[k] += a.sum(0)
                mags[k] += ma.sum(0)
    return out, mags


ROW_KEYS = ('rgb', 'g_feat')
SUM_KEYS = ('gW1', 'gb1', 'gW2', 'gb2', 'gW3', 'gb3')


def excess(got, ref, mag, k):
    """max over elements of |got - ref| / (k u mag); <= 1 means within the bound.  Non-finite `got` -> inf."""
    got = got.to(ref.device).double()
    err = (got - ref).abs()
    r = err / (k * U * mag).clamp_min(1e-300)
    r = torch.where(err == 0, torch.zeros_like(r), r)
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, float('inf')))
    return float(r.max()) if r.numel() else 0.0


def assert_close(name, got, ref, mag, k):
    e = excess(got, ref, mag, k)
    if not e <= 1.0:
        bad = ((got.to(ref.device).double() - ref).abs() > k * U * mag) | ~torch.isfinite(got.to(ref.device))
        idx = bad.nonzero()[:5].tolist()
        raise AssertionError(f'{name}: {int(bad.sum())} of {ref.numel()} elements outside {k} u * magnitude '
                             f'(worst {e:.3g} x the bound); first at {idx}')


def split_ties(margin, k=K_ROW):
    """Boolean [M]: rows whose every ReLU decision is clear of float32 rounding (margin >= k u)."""
    return margin >= k * U
