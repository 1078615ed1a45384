"""The float64 colour-head oracle (tests/shade_oracle.py) on the CPU, before any GPU test trusts it:
  - against float64 torch autograd of make_rgbnet(...).double(), for both forms, both widths and the edge inputs the GPU
    tests use (exactly-zero pre-activations, weights and features far from the default scale);
  - against the raw_rgb of the golden fixtures with a head (the reference's own float32 forward), within the same
    K_ROW u * magnitude bound the GPU kernels are held to.
"""
import numpy as np
import pytest
import torch

import shade_oracle as S
from conftest import load_golden


def _net(d_in, width, seed, w_scale=(1.0, 1.0, 1.0), zero_units=False):
    from directvoxgo_amd.dvgo import make_rgbnet
    torch.manual_seed(seed)
    net = make_rgbnet(d_in, width, 3).double()
    with torch.no_grad():
        for lin, s in zip((net[0], net[2][0], net[3]), w_scale):
            lin.weight.mul_(s)
            lin.bias.uniform_(-0.1 * s, 0.1 * s)
        if zero_units:            # units whose pre-activation is exactly +0 / -0 (all terms zero)
            net[0].weight[3].zero_(); net[0].bias[3] = 0.0
            net[0].weight[5].fill_(-0.0); net[0].bias[5] = -0.0
            net[2][0].weight[7].zero_(); net[2][0].bias[7] = -0.0
    return net


CASES = [  # width, diffuse, C, E, w_scale, feat_scale, zero_units
    (128, True, 12, 27, (1, 1, 1), 1.0, False),
    (128, False, 12, 27, (10, 0.1, 3), 1.0, False),
    (64, False, 9, 3, (1, 1, 1), 1e3, False),
    (64, True, 13, 3, (0.1, 10, 1), 1e-3, True),
    (128, True, 3, 15, (1, 1, 1), 1.0, True),        # diffuse head with no view features (n_view = 0)
]


@pytest.mark.parametrize('width,diffuse,C,E,w_scale,f_scale,zero_units', CASES)
def test_oracle_matches_float64_autograd(width, diffuse, C, E, w_scale, f_scale, zero_units):
    M, N = 3000, 37
    d_in = (C - 3 if diffuse else C) + E
    net = _net(d_in, width, seed=width + C + E, w_scale=w_scale, zero_units=zero_units)
    g = torch.Generator().manual_seed(5)
    feat = (torch.randn(M, C, generator=g, dtype=torch.float64) * f_scale)
    if zero_units:
        feat = feat.abs()                                # inputs of one sign: the -0 row gives -0 terms only
    emb = torch.rand(N, E, generator=g, dtype=torch.float64)
    ray_id = torch.randint(N, (M,), generator=g)
    go = torch.randn(M, 3, generator=g, dtype=torch.float64)
    P = S.params_of(net)
    out, mag = S.forward_backward(P, feat, emb, ray_id, go, diffuse)

    fr = feat.clone().requires_grad_(True)
    x = torch.cat([fr[:, 3:] if diffuse else fr, emb[ray_id]], -1)
    ref = torch.sigmoid(net(x) + (fr[:, :3] if diffuse else 0))
    grads = torch.autograd.grad(ref, [fr] + list(net.parameters()), go)
    names = ['rgb', 'g_feat', 'gW1', 'gb1', 'gW2', 'gb2', 'gW3', 'gb3']
    for name, r in zip(names, [ref.detach()] + list(grads)):
        err = (out[name] - r).abs()
        assert bool((err <= 1e-12 * mag[name]).all()), name
        assert bool((r.abs() <= mag[name] * (1 + 1e-12)).all()), f'{name}: magnitude below the value'
    if zero_units:
        # relu'(0) = 0 in torch: the dead units pass no gradient, whatever the sign of the zero
        assert out['margin'].min() > 0
        for u in (3, 5):
            assert float(out['gW1'][u].abs().max()) == 0 and float(out['gb1'][u]) == 0
        assert float(out['gW2'][7].abs().max()) == 0 and float(out['gb2'][7]) == 0
    # the forward-only entry gives the same rows
    rgb, rmag, margin = S.forward(P, feat, emb, ray_id, diffuse)
    assert torch.equal(rgb, out['rgb']) and torch.equal(rmag, mag['rgb']) and torch.equal(margin, out['margin'])


@pytest.mark.parametrize('name', ['forward_fine', 'forward_fine_direct', 'forward_mpi_w64'])
def test_oracle_matches_golden_raw_rgb(name, oracle):
    import render_oracle as R
    from test_render_oracle_host import render_kwargs, scene_of
    g = load_golden(name)
    sc = scene_of(g)
    out = R.forward(sc, g['rays_o'], g['rays_d'], g['viewdirs'], dtype=torch.float32, **render_kwargs(g))
    assert np.array_equal(out['ray_id'], g['out_ray_id'])
    P = [torch.from_numpy(np.asarray(a)).double() for _, W, b in sc.head for a in (W, b)]
    emb = out['_emb']
    assert emb.dtype == torch.float32
    feat = torch.from_numpy(out['feat'])
    rid = torch.from_numpy(out['ray_id'])
    rgb, mag, margin = S.forward(P, feat, emb, rid, not sc.direct)
    keep = S.split_ties(margin)
    print(f"{name}: {int((~keep).sum())} of {feat.shape[0]} rows dropped as ReLU ties")
    assert int(keep.sum()) >= 0.5 * feat.shape[0], f'{int((~keep).sum())} tie rows of {feat.shape[0]}'
    ref = torch.from_numpy(g['out_raw_rgb']).double()
    S.assert_close(name, ref[keep], rgb[keep], mag[keep], S.K_ROW)
    # and the bound is not vacuous: the float32 fixture is not the float64 value
    assert float((ref - rgb).abs().max()) > 0


def test_excess_and_ties_helpers():
    ref = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)
    mag = torch.tensor([1.0, 1.0, 0.0], dtype=torch.float64)
    assert S.excess(ref.float(), ref, mag, 1) == 0.0
    assert S.excess(torch.tensor([1.0, 2.0 + 2 ** -20, 3.0]), ref, mag, 1) == pytest.approx(16.0)
    assert S.excess(torch.tensor([1.0, float('nan'), 3.0]), ref, mag, 1) == float('inf')
    with pytest.raises(AssertionError, match='1 of 3 elements'):
        S.assert_close('x', torch.tensor([1.0, 2.0, 3.5]), ref, mag, S.K_ROW)
    m = torch.tensor([0.0, S.K_ROW * S.U * 0.5, S.K_ROW * S.U, float('inf')], dtype=torch.float64)
    assert S.split_ties(m).tolist() == [False, False, True, True]
