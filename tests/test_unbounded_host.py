"""Host-side checks of the unbounded-scene model (no GPU): the contraction, the sample-distance table, the distortion
loss's closed form against its definition, the model's constructor / kwargs / state dict, and the explicit errors of
what is out of scope."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unbounded_oracle as U  # noqa: E402

from directvoxgo_amd import dcvgo  # noqa: E402
from directvoxgo_amd.dcvgo import DirectContractedVoxGO  # noqa: E402


@pytest.mark.parametrize('norm', ['inf', 'l2'])
@pytest.mark.parametrize('b', [0.2, 0.5])
def test_contraction_continuous_and_bounded(norm, b):
    rng = np.random.default_rng(0)
    dirs = rng.normal(size=(512, 3)).astype(np.float32)
    n = np.maximum(np.abs(dirs).max(-1), 0) if norm == 'inf' else np.linalg.norm(dirs, axis=-1)
    unit = dirs / n[:, None].astype(np.float32)
    for eps in (1e-3, 1e-5):
        qi = U.contract(unit * np.float32(1 - eps), b, norm)[0]
        qo = U.contract(unit * np.float32(1 + eps), b, norm)[0]
        assert np.abs(qi - qo).max() < 4 * eps * (1 + b)
    far = unit[:, None, :] * np.logspace(0, 8, 50, dtype=np.float32)[None, :, None]
    q = U.contract(far.reshape(-1, 3), b, norm)[0]
    assert np.isfinite(q).all()
    assert np.abs(q).max() <= np.float32(1 + b)
    pts = rng.normal(scale=30, size=(4096, 3)).astype(np.float32)
    qn = U.contract(pts, b, norm)[1]
    q = U.contract(pts, b, norm)[0]
    assert np.abs(q).max() <= np.float32(1 + b)
    inner = qn <= 1
    assert np.array_equal(q[inner], pts[inner])


@pytest.mark.parametrize('world,stepsize,b', [(64, 0.5, 0.2), (160, 0.5, 0.2), (96, 1.0, 0.5), (33, 0.37, 0.5)])
def test_t_table(world, stepsize, b):
    t, n_in, n_max = dcvgo.contracted_t_table(world, stepsize, b)
    t_o, n_in_o, n_max_o = U.t_table(world, stepsize, b)
    assert np.array_equal(t, t_o) and t.dtype == np.float32
    assert n_in == int(np.floor(2 / (2 + 2 * b) * world / stepsize)) + 1 and n_max == 2 * n_in == n_max_o == t.shape[0]
    assert np.all(np.diff(t.astype(np.float64)) > 0)
    gaps = np.diff(t[:n_in].astype(np.float64))
    assert np.allclose(gaps, 2 / n_in, rtol=0, atol=2.4e-7)            # equal up to the float32 rounding of t (ulp(2))
    assert t[0] == np.float32(1 / n_in) and t[n_in - 1] < 2 < t[n_in]
    assert dcvgo.thinning_threshold(world, stepsize, b) == U.threshold(world, stepsize, b)


def _rand_segments(rng, n_rays, max_len):
    lens = rng.integers(0, max_len + 1, n_rays)
    lens[:3] = [0, 1, 2]
    ray_id = np.repeat(np.arange(n_rays), lens)
    w = rng.random(ray_id.shape[0]) * 0.3
    s = np.concatenate([np.sort(rng.random(n)) for n in lens]) if lens.sum() else np.zeros(0)
    return w, s, ray_id


def test_distortion_closed_form_equals_definition():
    rng = np.random.default_rng(1)
    w, s, ray_id = _rand_segments(rng, 40, 30)
    loss, grad = U.distortion(w, s, ray_id, 40, 97)
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    ref = U.distortion_n2(wt, torch.tensor(s, dtype=torch.float64), ray_id, 40, 97)
    ref.backward()
    assert loss == pytest.approx(ref.item(), rel=1e-12, abs=1e-15)
    np.testing.assert_allclose(grad, wt.grad.numpy(), rtol=1e-10, atol=1e-14)


def _model(**kw):
    args = dict(xyz_min=[-1, -2, -0.5], xyz_max=[1, 2, 1.5], num_voxels=24 ** 3, num_voxels_base=24 ** 3,
                alpha_init=1e-2, bg_len=0.2)
    args.update(kw)
    return DirectContractedVoxGO(**args)


@pytest.mark.parametrize('rgbnet_dim,direct', [(0, True), (12, True), (12, False)])
def test_model_construct_kwargs_state_dict(rgbnet_dim, direct):
    m = _model(rgbnet_dim=rgbnet_dim, rgbnet_direct=direct, contracted_norm='l2')
    assert tuple(m.density.shape) == (1, 1, 24, 24, 24)
    assert m.k0.shape[1] == (3 if rgbnet_dim == 0 else 12)
    assert torch.equal(m.scene_center, torch.tensor([0., 0., 0.5])) and torch.equal(m.scene_radius, torch.tensor([1., 2., 1.]))
    assert torch.allclose(m.xyz_min, torch.full((3,), -1.2)) and torch.allclose(m.xyz_max, torch.full((3,), 1.2))
    assert tuple(m.mask_cache.mask.shape) == (24, 24, 24)
    kw = m.get_kwargs()
    assert np.array_equal(kw['xyz_min'], np.float32([-1, -2, -0.5])) and kw['contracted_norm'] == 'l2' and kw['bg_len'] == 0.2
    from directvoxgo_amd.checkpoint import model_kwargs_of
    with torch.no_grad():
        m.density.normal_()
        m.k0.normal_()
    m2 = DirectContractedVoxGO(**model_kwargs_of({'model_kwargs': kw}))
    m2.load_state_dict(m.state_dict())
    for k, v in m.state_dict().items():
        assert torch.equal(v, m2.state_dict()[k]), k


def test_out_of_scope_raises(tmp_path):
    with pytest.raises(NotImplementedError):
        _model(rgbnet_dim=12, posbase_pe=5)
    m = _model()
    from directvoxgo_amd.export import extract_mesh
    with pytest.raises(NotImplementedError):
        extract_mesh(m)
    from directvoxgo_amd.fit import fit_stage
    from directvoxgo_amd.train import COARSE_TRAIN
    cfg = dict(COARSE_TRAIN, pervoxel_lr=True)
    z = torch.zeros((4, 3))
    with pytest.raises(ValueError):
        fit_stage(m, z, z, z, z, cfg, dict(near=0, far=1, stepsize=0.5, bg=0), n_iters=1, imsz=[4])
    with pytest.raises(NotImplementedError):
        m.voxel_count_views(z, z, [4], 0, 1, 0.5)
