"""The colour head kernels (csrc/shade_x3.hip, csrc/shade.hip) against the float64 oracle of tests/shade_oracle.py, on the
default kernel variant 67 (bf16 3-way split forward / data gradient, split-operand ring weight gradient) and on variant 0
(fp32 MFMA throughout).

Every value, data gradient and weight / bias gradient is held elementwise to K * 2^-24 * magnitude (shade_oracle.py
justifies K).  Each batch is drawn tie-free first: candidate rows whose ReLU margin is within the bound are dropped, so no
norm fallback is needed.  Most cases call the C ABI the way directvoxgo_amd/shade.py does, but with arrays the test owns.
That way the capacity-mode sentinels and the saved activations can be read.

Dispatch branch -> case id that reaches it (both variants unless noted):
  x3 forward, width 64, KS=1 (d_in <= 16) / KS=3      branch[w64-direct-C13-E3-dIn16] / [w64-direct-C14-E3-dIn17]
  f32 forward, width 128, S1=18 (d_in <= 36) / 20      branch[w128-diffuse-C12-E27-dIn36] / [w128-diffuse-C13-E27-dIn37]
  f32 forward, width 64, S1=6 (d_in <= 12) / 20        branch[w64-direct-C9-E3-dIn12] / [w64-diffuse-C13-E3-dIn13]
  ring wgrad, first clause n_view + E == 32 / <= 32    branch[w128-direct-C11-E21-dIn32] / [w64-diffuse-C12-E21-dIn30]
  ring wgrad, width 64 via n_view % 4 == 0, n_view>=8  branch[w64-direct-C12-E27-dIn39], [w64-direct-C12-E21-dIn33]
  r1 wgrad (predicate false): n_view + E == 33         branch[w128-diffuse-C9-E27-dIn33], E = 33: [w64-diffuse-C3-E33-dIn33]
  ring wgrad / r1 at the 2^31-byte switch (width 128)  test_wgrad_2g_switch[4194303] / [4194335]
  ring wgrad, n_parts clamped at 512 (M > 131072)      test_partition_edges[*-131073], [*-300001]
  shade() with n_view = 0 (diffuse, C = 3)             branch[w64-diffuse-C3-E33-dIn33], branch[w128-diffuse-C3-E15-dIn15]
  m_dev capacity mode (all kernels)                    test_capacity_mode
"""
import time

import numpy as np
import pytest
import torch

import shade_oracle as S

pytestmark = pytest.mark.gpu

VARIANTS = [67, 0]
SENT = 12345.0                       # sentinel of the float outputs past m (capacity mode)
SENT_MASK = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(params=VARIANTS, ids=lambda v: f'v{v}')
def variant(request):
    from directvoxgo_amd import _lib as L
    prev = L.lib().dvgo_shade_variant(request.param)
    yield request.param
    L.lib().dvgo_shade_variant(prev)


# ------------------------------------------------------------------ inputs
def make_params(d_in, width, seed, w_scale=(1.0, 1.0, 1.0)):
    """fp32 (W1, b1, W2, b2, W3, b3) on the GPU: make_rgbnet's init, weights scaled per layer, non-zero biases."""
    from directvoxgo_amd.dvgo import make_rgbnet
    torch.manual_seed(seed)
    net = make_rgbnet(d_in, width, 3)
    with torch.no_grad():
        for lin, s in zip((net[0], net[2][0], net[3]), w_scale):
            lin.weight.mul_(s)
            lin.bias.uniform_(-0.1 * s, 0.1 * s)
    return [t.detach().cuda().contiguous() for t in (net[0].weight, net[0].bias, net[2][0].weight, net[2][0].bias,
                                                     net[3].weight, net[3].bias)]


def make_batch(P, M, C, E, diffuse, seed, f_scale=None, rays='sorted', n_rays=50, positive=False):
    """M tie-free rows: feat [M,C], emb [N,E], ray_id [M], g_rgb [M,3], plus the number of candidate rows dropped.
    f_scale None: randn features; a pair (lo, hi): each row scaled by a log-uniform factor in [lo, hi]."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    n = M + M // 3 + 64
    feat = torch.randn(n, C, device='cuda', generator=g)
    if f_scale is not None:
        lo, hi = np.log10(f_scale[0]), np.log10(f_scale[1])
        feat = feat * 10.0 ** (torch.rand(n, 1, device='cuda', generator=g) * (hi - lo) + lo)
    if positive:
        feat = feat.abs()
    N = n if rays == 'per_row' else n_rays
    emb = torch.rand(N, E, device='cuda', generator=g) * (1.0 if positive else 2.0) - (0.0 if positive else 1.0)
    if rays == 'per_row':
        ray_id = torch.arange(n, device='cuda')
    elif rays == 'one':
        ray_id = torch.full((n,), N // 2, device='cuda', dtype=torch.int64)
    else:
        ray_id = torch.randint(N, (n,), device='cuda', generator=g)
        if rays == 'sorted':
            ray_id = torch.sort(ray_id)[0]
    g_rgb = torch.randn(n, 3, device='cuda', generator=g)
    _, _, margin = S.forward([p.double() for p in P], feat, emb, ray_id, diffuse)
    keep = S.split_ties(margin).nonzero()[:, 0]
    assert keep.numel() >= M, f'only {keep.numel()} tie-free rows of {n}'
    dropped = int((S.split_ties(margin)[:int(keep[M - 1]) + 1] == 0).sum())
    keep = keep[:M]
    return feat[keep].contiguous(), emb.contiguous(), ray_id[keep].contiguous(), g_rgb[keep].contiguous(), dropped


# ------------------------------------------------------------------ the kernels through the C ABI (as shade.py calls them)
def run(P, feat, emb, ray_id, g_rgb, diffuse, m_dev=None, sentinel=False, wgrad=True):
    """dict: rgb, H1, H2, masks, g_feat, G1, gz and (wgrad) gW1 gb1 gW2 gb2 gW3 gb3, all on the GPU."""
    from directvoxgo_amd import _lib as L
    from directvoxgo_amd._lib import _i64, _int, ptr, stream_of
    from directvoxgo_amd.shade import N_PARTS, _scratch
    W1, b1, W2, b2, W3, b3 = P
    M, C = feat.shape
    E = emb.shape[1]
    width, d_in = W1.shape
    dev = feat.device
    new = (lambda *s: torch.full(s, SENT, device=dev)) if sentinel else (lambda *s: torch.empty(s, device=dev))
    o = dict(rgb=new(M, 3), H1=new(M, width), H2=new(M, width), g_feat=new(M, C), G1=new(M, width), gz=new(M, 3))
    o['masks'] = torch.full((M, 4), SENT_MASK, dtype=torch.int64, device=dev)
    variant = L.lib().dvgo_shade_variant(-1)
    scratch = _scratch(width, dev)
    scratch_bwd = _scratch(width, dev) if variant & 2 else None
    d = 1 if diffuse else 0
    st = stream_of(feat)
    L.call('dvgo_shade_fwd', ptr(feat), _int(C), ptr(emb), _int(E), ptr(ray_id), _i64(M), ptr(m_dev), ptr(W1), ptr(b1),
           ptr(W2), ptr(b2), ptr(W3), ptr(b3), _int(width), _int(d_in), _int(d), ptr(o['rgb']), ptr(o['H1']), ptr(o['H2']),
           ptr(o['masks']), ptr(scratch), ptr(scratch_bwd), st)
    prebuilt = scratch_bwd is not None and (variant & 1)
    L.call('dvgo_shade_bwd', ptr(g_rgb), ptr(o['rgb']), ptr(o['masks']), _i64(M), ptr(m_dev), ptr(W1), ptr(W2), ptr(W3),
           _int(width), _int(d_in), _int(C), _int(d), ptr(o['g_feat']), ptr(o['G1']), ptr(o['gz']),
           ptr(scratch_bwd if prebuilt else _scratch(width, dev)), _int(1 if prebuilt else 0), st)
    if wgrad:
        n_parts = max(1, min(N_PARTS, (M + 255) // 256))
        part = torch.empty((n_parts, width * width + width * 64 + 32 * width + 3 * width), device=dev)
        tot = torch.empty(width * width + width * d_in + 5 * width + 3, device=dev)
        L.call('dvgo_shade_wgrad', ptr(o['G1']), ptr(o['gz']), ptr(o['masks']), ptr(W3), ptr(o['H1']), ptr(o['H2']),
               ptr(feat), _int(C), ptr(emb), _int(E), ptr(ray_id), _i64(M), ptr(m_dev), _int(width), _int(d), _int(n_parts),
               ptr(part), ptr(tot), st)
        k = 0
        for name, shape in (('gW2', (width, width)), ('gW1', (width, d_in)), ('gW3', (3, width)), ('gb1', (width,)),
                            ('gb2', (width,)), ('gb3', (3,))):
            n = int(np.prod(shape))
            o[name] = tot[k:k + n].view(shape)
            k += n
    torch.cuda.synchronize()
    return o


def check(P, feat, emb, ray_id, g_rgb, diffuse, got=None, rows=None):
    """Hold every output of `got` (default: a fresh run) to the oracle; `rows`: only the first `rows` rows count."""
    got = run(P, feat, emb, ray_id, g_rgb, diffuse) if got is None else got
    m = feat.shape[0] if rows is None else rows
    ref, mag = S.forward_backward([p.double() for p in P], feat[:m], emb, ray_id[:m], g_rgb[:m], diffuse)
    for k in S.ROW_KEYS:
        S.assert_close(k, got[k][:m], ref[k], mag[k], S.K_ROW)
    for k in S.SUM_KEYS:
        S.assert_close(k, got[k], ref[k], mag[k], S.K_SUM)
    return got


# ------------------------------------------------------------------ branch matrix
BRANCH = [  # width, diffuse, C, E
    (64, False, 13, 3), (64, False, 14, 3),            # x3 KS=1 / KS=3 boundary (d_in 16 / 17; C=14 is the only way to 17)
    (128, True, 12, 27), (128, True, 13, 27),          # f32 S1 = 18 / 20 at width 128 (d_in 36 / 37)
    (128, False, 12, 27),                              # the default rgbnet_direct head (d_in 39)
    (64, False, 9, 3), (64, True, 13, 3),              # f32 S1 = 6 / 20 at width 64 (d_in 12 / 13)
    (128, False, 11, 21),                              # ring, n_view + E == 32 (C = 11: the set has no 32)
    (64, True, 12, 21),                                # ring, n_view + E = 30
    (64, False, 12, 27), (64, False, 12, 21),          # ring at width 64 via n_view % 4 == 0 (d_in 39 and 33)
    (128, True, 9, 27),                                # r1: n_view + E == 33, n_view = 6
    (64, True, 3, 33), (128, True, 3, 15),             # n_view = 0 (diffuse C = 3); E = 33 > 32 -> r1
    (128, False, 9, 9), (64, True, 9, 15),
]


def _bid(c):
    w, diffuse, C, E = c
    return f"w{w}-{'diffuse' if diffuse else 'direct'}-C{C}-E{E}-dIn{C - (3 if diffuse else 0) + E}"


@pytest.mark.parametrize('width,diffuse,C,E', BRANCH, ids=[_bid(c) for c in BRANCH])
def test_branch(variant, width, diffuse, C, E):
    d_in = C - (3 if diffuse else 0) + E
    P = make_params(d_in, width, seed=width * 100 + C * 3 + E)
    feat, emb, rid, g, _ = make_batch(P, 2000, C, E, diffuse, seed=C + E)
    check(P, feat, emb, rid, g, diffuse)


def test_branch_through_shade_autograd(variant):
    """The same oracle through directvoxgo_amd.shade.shade and autograd (the path training takes), n_view = 0."""
    from directvoxgo_amd.dvgo import make_rgbnet
    from directvoxgo_amd.shade import shade
    P = make_params(15, 128, seed=3)
    feat, emb, rid, g, _ = make_batch(P, 3000, 3, 15, True, seed=4)
    net = make_rgbnet(15, 128, 3).cuda()
    with torch.no_grad():
        for p, q in zip(net.parameters(), P):
            p.copy_(q)
    f = feat.clone().requires_grad_(True)
    rgb = shade(net, f, emb, rid, True)
    assert rgb is not None
    grads = torch.autograd.grad(rgb, [f] + list(net.parameters()), g)
    got = dict(rgb=rgb.detach(), g_feat=grads[0], **dict(zip(('gW1', 'gb1', 'gW2', 'gb2', 'gW3', 'gb3'), grads[1:])))
    check(P, feat, emb, rid, g, True, got=got)


# ------------------------------------------------------------------ partition edges
EDGE_M = [1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 131072, 131073, 300001]


@pytest.mark.parametrize('shape', [(128, True, 12, 27), (64, False, 9, 3)], ids=['w128-diffuse', 'w64-direct'])
@pytest.mark.parametrize('M', EDGE_M)
def test_partition_edges(variant, shape, M):
    """32-row forward tiles, 16-row ring tiles, n_parts = ceil(M / 256) up to its clamp at 512 (M > 131072)."""
    width, diffuse, C, E = shape
    P = make_params(C - (3 if diffuse else 0) + E, width, seed=11)
    feat, emb, rid, g, _ = make_batch(P, M, C, E, diffuse, seed=M)
    check(P, feat, emb, rid, g, diffuse)


@pytest.mark.parametrize('M', [4194303, 4194335])
def test_wgrad_2g_switch(variant, M, capsys):
    """M * width * 4 < 2^31 selects the ring weight-gradient kernel, else the r1 kernel: 4 194 303 rows are the last
    ring batch at width 128, 4 194 335 take r1.  Both are held to the oracle."""
    t0 = time.time()
    P = make_params(39, 128, seed=21)
    feat, emb, rid, g, dropped = make_batch(P, M, 12, 27, False, seed=22, n_rays=8192)
    t1 = time.time()
    check(P, feat, emb, rid, g, False)
    with capsys.disabled():
        print(f'\n[2g switch M={M} v{variant}] batch {t1 - t0:.1f} s ({dropped} tie rows dropped), '
              f'kernels + oracle {time.time() - t1:.1f} s')


# ------------------------------------------------------------------ position independence
def test_rows_are_position_independent(variant):
    """A row's rgb and g_feat have the same bits whatever M is and wherever the row sits."""
    width, diffuse, C, E = 128, True, 12, 27
    P = make_params(36, width, seed=31)
    feat, emb, rid, g, _ = make_batch(P, 1000 + 33, C, E, diffuse, seed=32)
    base = run(P, feat[33:], emb, rid[33:], g[33:], diffuse, wgrad=False)
    for k in (1, 17, 33):
        o = run(P, feat[33 - k:], emb, rid[33 - k:], g[33 - k:], diffuse, wgrad=False)
        assert torch.equal(o['rgb'][k:], base['rgb']) and torch.equal(o['g_feat'][k:], base['g_feat']), k
    M = 1000
    perm = torch.cat([torch.arange(M // 2, M), torch.arange(M // 2)]).cuda()
    o = run(P, feat[33:][perm], emb, rid[33:][perm], g[33:][perm], diffuse, wgrad=False)
    assert torch.equal(o['rgb'], base['rgb'][perm]) and torch.equal(o['g_feat'], base['g_feat'][perm])


# ------------------------------------------------------------------ inputs away from randn
@pytest.mark.parametrize('w_scale', [(10, 0.1, 1), (0.1, 10, 3), (3, 3, 0.1)], ids=str)
@pytest.mark.parametrize('shape', [(128, False, 12, 27), (64, True, 12, 3)], ids=['w128-direct', 'w64-diffuse'])
def test_trained_weight_scales(variant, shape, w_scale):
    width, diffuse, C, E = shape
    P = make_params(C - (3 if diffuse else 0) + E, width, seed=41, w_scale=w_scale)
    feat, emb, rid, g, _ = make_batch(P, 5000, C, E, diffuse, seed=42)
    check(P, feat, emb, rid, g, diffuse)


@pytest.mark.parametrize('rays', ['sorted', 'unsorted', 'one', 'per_row'])
def test_feature_magnitudes_and_ray_layouts(variant, rays):
    """Features of magnitude 1e-3 .. 1e3 (per row, log-uniform); sorted / unsorted ray ids, one ray, one ray per row."""
    width, diffuse, C, E = 128, True, 12, 27
    P = make_params(36, width, seed=51)
    feat, emb, rid, g, _ = make_batch(P, 5000, C, E, diffuse, seed=52, f_scale=(1e-3, 1e3), rays=rays)
    check(P, feat, emb, rid, g, diffuse)


# ------------------------------------------------------------------ capacity mode
@pytest.mark.parametrize('shape', [(128, True, 12, 27), (128, False, 12, 27), (64, False, 12, 27)],
                         ids=['w128-diffuse-r1', 'w128-direct-ring', 'w64-direct-ring'])
def test_capacity_mode(variant, shape):
    """Arrays sized M_cap, the sample count on the device (fused.py capacity mode).  Rows >= m hold NaN inputs; the
    kernels must neither read nor write them."""
    width, diffuse, C, E = shape
    P = make_params(C - (3 if diffuse else 0) + E, width, seed=61)
    M_cap = 700
    feat, emb, rid, g, _ = make_batch(P, M_cap, C, E, diffuse, seed=62)
    for m in (0, 333, 10 ** 9):
        mm = min(m, M_cap)
        f, gg, r = feat.clone(), g.clone(), rid.clone()
        f[mm:] = float('nan')
        gg[mm:] = float('nan')
        r[mm:] = 0                    # (a valid row of emb: a kernel that did read past m stays in bounds)
        m_dev = torch.tensor([m], dtype=torch.int64, device='cuda')
        o = run(P, f, emb, r, gg, diffuse, m_dev=m_dev, sentinel=True)
        for k in ('rgb', 'H1', 'H2', 'G1', 'gz', 'g_feat'):
            assert bool((o[k][mm:] == SENT).all()), f'm={m}: {k} written past m'
        assert bool((o['masks'][mm:] == SENT_MASK).all()), f'm={m}: masks written past m'
        for k in S.SUM_KEYS:
            assert bool(torch.isfinite(o[k]).all()), f'm={m}: {k} not finite'
        if mm == 0:
            for k in S.SUM_KEYS:
                assert float(o[k].abs().max()) == 0.0, f'm=0: {k} not zero'
            continue
        ref = run(P, feat[:mm].contiguous(), emb, rid[:mm].contiguous(), g[:mm].contiguous(), diffuse, wgrad=False)
        assert torch.equal(o['rgb'][:mm], ref['rgb']) and torch.equal(o['g_feat'][:mm], ref['g_feat']), f'm={m}'
        check(P, feat, emb, rid, g, diffuse, got=o, rows=mm)


# ------------------------------------------------------------------ exactly-zero pre-activations
@pytest.mark.parametrize('shape', [(128, True, 12, 27), (64, False, 9, 3)], ids=['w128-diffuse', 'w64-direct'])
def test_zero_preactivations_pass_no_gradient(variant, shape):
    """Units whose pre-activation is exactly +0 or -0 (every term zero: rows of zeros / negative zeros, biases +0 / -0,
    inputs of one sign), in layer 1 and in layer 2.  relu'(0) = 0 in torch: they must contribute no gradient."""
    width, diffuse, C, E = shape
    d_in = C - (3 if diffuse else 0) + E
    P = make_params(d_in, width, seed=71)
    W1, b1, W2, b2, W3, b3 = P
    W1[3] = 0.0; b1[3] = 0.0                       # layer 1, +0
    W1[5] = -0.0; b1[5] = -0.0                     # layer 1, -0 (inputs >= 0)
    W2[7] = -0.0; b2[7] = -0.0                     # layer 2, -0 (post-ReLU inputs >= 0)
    W2[9] = 0.0; b2[9] = 0.0                       # layer 2, +0
    assert torch.signbit(W1[5]).all() and torch.signbit(b2[7])
    feat, emb, rid, g, _ = make_batch(P, 3000, C, E, diffuse, seed=72, positive=True)
    o = check(P, feat, emb, rid, g, diffuse)
    for u in (3, 5):
        assert float(o['gW1'][u].abs().max()) == 0 and float(o['gb1'][u].abs()) == 0, f'layer-1 unit {u}'
        assert float(o['G1'][:, u].abs().max()) == 0, f'layer-1 unit {u}'
        assert float(o['gW2'][:, u].abs().max()) == 0
    for v in (7, 9):
        assert float(o['gW2'][v].abs().max()) == 0 and float(o['gb2'][v].abs()) == 0, f'layer-2 unit {v}'
        assert float(o['gW3'][:, v].abs().max()) == 0


# ------------------------------------------------------------------ non-finite inputs
@pytest.mark.parametrize('shape', [(128, True, 12, 27), (64, False, 9, 3)], ids=['w128-diffuse', 'w64-direct'])
def test_non_finite_feature_propagates(variant, shape):
    """One row with an inf feature, one with a NaN feature.  As in torch, their colour and feature gradient are not
    finite and the weight gradients are not all finite (a diverging grid does not train on silently).  Every other
    row is bit for bit what it is without them."""
    width, diffuse, C, E = shape
    d_in = C - (3 if diffuse else 0) + E
    P = make_params(d_in, width, seed=81)
    feat, emb, rid, g, _ = make_batch(P, 1000, C, E, diffuse, seed=82)
    clean = run(P, feat, emb, rid, g, diffuse)
    bad = {100: float('inf'), 200: float('nan')}
    f = feat.clone()
    for r, v in bad.items():
        f[r, C - 1] = v                                # a view feature: it enters the MLP in both forms
    o = run(P, f, emb, rid, g, diffuse)
    other = torch.ones(f.shape[0], dtype=torch.bool, device='cuda')
    other[list(bad)] = False
    assert torch.equal(o['rgb'][other], clean['rgb'][other])
    assert torch.equal(o['g_feat'][other], clean['g_feat'][other])
    # torch float32 on the same rows
    W1, b1, W2, b2, W3, b3 = P
    fr = f.clone().requires_grad_(True)
    x = torch.cat([fr[:, 3:] if diffuse else fr, emb[rid]], -1)
    z = torch.relu(torch.relu(x @ W1.t() + b1) @ W2.t() + b2) @ W3.t() + b3
    ref = torch.sigmoid(z + (fr[:, :3] if diffuse else 0))
    (g_ref,) = torch.autograd.grad(ref, [fr], g)
    for r in bad:
        assert not bool(torch.isfinite(ref[r]).any()), 'premise: torch gives no finite colour on the row'
        assert torch.equal(torch.isfinite(o['rgb'][r]), torch.isfinite(ref[r])), f'row {r}: rgb {o["rgb"][r].tolist()}'
        assert torch.equal(torch.isfinite(o['g_feat'][r]), torch.isfinite(g_ref[r])), \
            f'row {r}: g_feat {o["g_feat"][r].tolist()} vs torch {g_ref[r].tolist()}'
    for k in S.SUM_KEYS:
        assert not bool(torch.isfinite(o[k]).all()), f'{k} is finite: the non-finite rows vanished'
