"""CPU: the positional-encoding colour head option (posbase_pe > 0) of DirectVoxGO -- constructor, state_dict, kwargs,
a reference-written checkpoint, and the float64 oracle (tests/posenc_oracle.py) pinned against the reference's own
colour head output (tests/golden/make_golden_posenc.py)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

import posenc_oracle as PO

FIXTURES = ('forward_fine_posenc', 'forward_fine_posenc_p4')


def _model_of(z, **over):
    from directvoxgo_amd.dvgo import DirectVoxGO
    P = int(z['posbase_pe'])
    kw = dict(num_voxels=int(np.prod(z['world_size'])), num_voxels_base=int(np.prod(z['world_size'])), alpha_init=1e-2,
              fast_color_thres=float(z['fast_color_thres']), rgbnet_dim=12, rgbnet_depth=3, rgbnet_width=128, viewbase_pe=4,
              rgbnet_direct=P == 10, posbase_pe=P)
    kw.update(over)
    return DirectVoxGO(z['xyz_min'], z['xyz_max'], **kw)


@pytest.mark.parametrize('name', FIXTURES)
def test_constructor_state_dict_and_kwargs(name):
    z = load_golden(name)
    P = int(z['posbase_pe'])
    m = _model_of(z)
    sd = m.state_dict()
    # lib/dvgo.py:97-107: posfreq only with a colour head and P > 0; k0 keeps its rgbnet_dim channels
    expect = {'xyz_min', 'xyz_max', 'density', 'k0', 'viewfreq', 'posfreq', 'rgbnet.0.weight', 'rgbnet.0.bias',
              'rgbnet.2.0.weight', 'rgbnet.2.0.bias', 'rgbnet.3.weight', 'rgbnet.3.bias', 'mask_cache.mask',
              'mask_cache.xyz2ijk_scale', 'mask_cache.xyz2ijk_shift'}
    assert set(sd) == expect
    assert torch.equal(sd['posfreq'], torch.tensor([2.0 ** i for i in range(P)]))
    d_in = (3 + 6 * 4) + (3 + 6 * P)                       # whatever rgbnet_direct says
    assert tuple(sd['rgbnet.0.weight'].shape) == tuple(z['rgbnet_0.weight'].shape) == (128, d_in)
    assert sd['k0'].shape[1] == 12 and tuple(sd['k0'].shape[2:]) == tuple(z['world_size'])
    assert m.uses_posenc and not m.can_keep_count_on_device()
    kw = m.get_kwargs()
    assert kw['posbase_pe'] == P
    m2 = type(m)(**kw)                                   # kwargs round trip (lib/utils.py:63-79)
    assert m2.posbase_pe == P and set(m2.state_dict()) == expect


def test_other_models_are_unchanged():
    """posbase_pe = 0 (and the coarse stage, where P has no effect): no posfreq buffer, no new kwargs key."""
    from directvoxgo_amd.dvgo import DirectVoxGO
    base = dict(num_voxels=8 ** 3, num_voxels_base=8 ** 3, alpha_init=1e-2)
    fine = DirectVoxGO([-1] * 3, [1] * 3, rgbnet_dim=12, **base)
    assert 'posbase_pe' not in fine.get_kwargs() and 'posfreq' not in fine.state_dict() and not fine.uses_posenc
    assert fine.rgbnet[0].in_features == 27 + 9
    coarse = DirectVoxGO([-1] * 3, [1] * 3, posbase_pe=10, **base)
    assert 'posfreq' not in coarse.state_dict() and coarse.rgbnet is None and not coarse.uses_posenc


def test_out_of_scope_options_still_raise():
    from directvoxgo_amd.dvgo import DirectVoxGO
    base = dict(num_voxels=8 ** 3, num_voxels_base=8 ** 3, alpha_init=1e-2, rgbnet_dim=12)
    with pytest.raises(NotImplementedError, match='rgbnet_full_implicit'):
        DirectVoxGO([-1] * 3, [1] * 3, rgbnet_full_implicit=True, posbase_pe=10, **base)
    with pytest.raises(NotImplementedError, match='implicit_voxel_feat'):
        DirectVoxGO([-1] * 3, [1] * 3, implicit_voxel_feat=True, **base)


def test_reference_posenc_checkpoint_loads():
    from directvoxgo_amd.checkpoint import load_model, safe_load
    from directvoxgo_amd.dvgo import DirectVoxGO
    path = os.path.join(GOLDEN, 'ref_checkpoint_posenc.tar')
    ck = safe_load(path)
    sd = ck['model_state_dict']
    assert ck['model_kwargs']['posbase_pe'] == 10
    m = load_model(DirectVoxGO, path)
    assert m.posbase_pe == 10 and m.uses_posenc
    got = m.state_dict()
    assert set(got) == set(sd), set(got) ^ set(sd)
    assert torch.equal(got['posfreq'], sd['posfreq'])
    assert tuple(got['rgbnet.0.weight'].shape) == (128, 90) and torch.equal(got['rgbnet.0.weight'], sd['rgbnet.0.weight'])
    assert torch.equal(m.k0.detach().contiguous(), sd['k0'])
    # the reference's MaskedAdam never saw a k0 gradient: no state for it (params: density 0, k0 1, rgbnet 2..7)
    assert 1 not in ck['optimizer_state_dict']['state'] and 0 in ck['optimizer_state_dict']['state']


@pytest.mark.parametrize('P,E', [(4, 6), (4, 27)], ids=['dIn33', 'dIn54'])
def test_oracle_rows_equal_float64_autograd(P, E):
    """PO.rows against float64 torch autograd on the module tree, one odd and one even d_in: hooks on the two ReLUs give
    h1 and h2, the gradients with respect to z1 and z3 give G1 and gz.  Both sides are float64 statements of the same
    chain: they agree to float64 rounding, far inside anything float32 could tell apart."""
    from directvoxgo_amd.dvgo import make_rgbnet
    torch.manual_seed(7 + P + E)
    M, N, d_in = 300, 17, 3 + 6 * P + E
    net = make_rgbnet(d_in, 128, 3).double()
    with torch.no_grad():
        for p in net.parameters():
            p.add_(torch.randn_like(p) * 0.05)
    pts = torch.rand(M, 3) * 3 - 1.5
    freq = torch.tensor([2.0 ** i for i in range(P)])
    emb = torch.rand(N, E) * 2 - 1
    rid = torch.randint(N, (M,))
    g = torch.randn(M, 3)
    seen = {}
    hooks = [net[0].register_forward_hook(lambda mod, i, o: (seen.__setitem__('z1', o), o.clone())[1]),   # (ReLU is in place)
             net[1].register_forward_hook(lambda mod, i, o: seen.__setitem__('h1', o.detach().clone())),
             net[2][1].register_forward_hook(lambda mod, i, o: seen.__setitem__('h2', o.detach().clone()))]
    x = torch.cat([PO.pos_embed(pts, freq), emb.double()[rid]], -1)
    z3 = net(x)
    for h in hooks:
        h.remove()
    rgb = torch.sigmoid(z3)
    G1, gz = torch.autograd.grad(rgb, [seen['z1'], z3], g.double())
    ref = dict(rgb=rgb.detach(), h1=seen['h1'], h2=seen['h2'], gz=gz, G1=G1)
    out, mags = PO.rows(PO.params_of(net), pts, freq, emb, rid, g)
    assert set(mags) == set(PO.ROW_KEYS) and set(out) == set(PO.ROW_KEYS) | {'k1', 'k2', 'margin'}
    for k in PO.ROW_KEYS:
        assert out[k].dtype == torch.float64 and out[k].shape == ref[k].shape == mags[k].shape, k
        assert bool((mags[k] >= out[k].abs() * (1 - 1e-12)).all()), k        # a magnitude bounds its value
        assert bool(((out[k] - ref[k]).abs() <= 1e-12 * mags[k]).all()), k
    assert torch.equal(out['k1'], seen['z1'].detach() > 0) and torch.equal(out['k1'], ref['h1'] > 0)
    assert torch.equal(out['k2'], ref['h2'] > 0)
    assert 0.2 < float(out['k1'].double().mean()) < 0.8 and 0.2 < float(out['k2'].double().mean()) < 0.8
    # the margin is forward()'s, and the batch sums of forward_backward are sums of these rows
    assert torch.equal(out['margin'], PO.forward(PO.params_of(net), pts, freq, emb, rid)[2])
    full, _ = PO.forward_backward(PO.params_of(net), pts, freq, emb, rid, g)
    assert torch.allclose(full['gb1'], out['G1'].sum(0), rtol=1e-12, atol=1e-14)
    assert torch.allclose(full['gb3'], out['gz'].sum(0), rtol=1e-12, atol=1e-14)
    assert torch.allclose(full['gW1'], out['G1'].t() @ x.detach(), rtol=1e-10, atol=1e-13)
    # an empty batch has empty rows of the right shapes
    e, em = PO.rows(PO.params_of(net), pts[:0], freq, emb, rid[:0], g[:0])
    assert e['rgb'].shape == (0, 3) and e['G1'].shape == (0, 128) and e['k1'].dtype == torch.bool and em['gz'].shape == (0, 3)


@pytest.mark.parametrize('name', FIXTURES)
def test_oracle_reproduces_the_reference_head(name):
    """The fixture keeps the rows the reference fed its colour head (positions first): the oracle's position encoding
    equals their encoding columns to float32 rounding, and its rgb from the positions equals the reference's raw_rgb
    within the oracle's own bound.  Pins the oracle."""
    z = load_golden(name)
    P = int(z['posbase_pe'])
    x = torch.from_numpy(z['head_input'])
    npos = 3 + 6 * P
    pts = x[:, :3]
    freq = torch.tensor([2.0 ** i for i in range(P)])
    enc = PO.pos_embed(pts, freq)
    assert torch.equal(enc[:, :3].float(), pts)
    assert (enc - x[:, :npos].double()).abs().max() <= 2 * 2.0 ** -24       # torch's float32 sin / cos: within an ulp
    # one row per kept sample, in the order of raw_rgb
    M = z['out_raw_rgb'].shape[0]
    assert x.shape == (M, npos + 27)
    params = [torch.from_numpy(z['rgbnet_' + k]).double() for k in
              ('0.weight', '0.bias', '2.0.weight', '2.0.bias', '3.weight', '3.bias')]
    emb = x[:, npos:]                                            # viewdirs_emb[ray_id], as the reference formed it
    ve = PO.view_embed(torch.from_numpy(z['viewdirs']), torch.tensor([1.0, 2.0, 4.0, 8.0]))
    rid = torch.from_numpy(z['out_ray_id'])
    assert (ve[rid] - emb.double()).abs().max() <= 2 * 2.0 ** -24
    rgb, mag, margin = PO.forward(params, pts, freq, emb, torch.arange(M))
    ref = torch.from_numpy(z['out_raw_rgb']).double()
    PO.assert_close('raw_rgb', ref, rgb, mag, PO.K_ROW)
    assert (rgb - ref).abs().max() < 1e-5
