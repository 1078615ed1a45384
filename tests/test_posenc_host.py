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
