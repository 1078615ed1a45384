"""The CPU render oracle (tests/render_oracle.py) against the golden forward fixtures: the reference's own
lib/dvgo.py / lib/dmpigo.py orchestration over the oracle natives (tests/golden/make_golden.py).  The full-size GPU
tests (tests/test_gpu_fullsize_oracle.py) trust the helper only as far as this file pins it: ids exactly, values and
gradients to the tolerances of test_gpu_forward.py::test_forward_matches_reference_orchestration, with the float32
head and with the float64 arbiter head."""
import numpy as np
import pytest
import torch

from conftest import load_golden

FIXTURES = ['forward_coarse', 'forward_fine', 'forward_fine_direct', 'forward_mpi', 'forward_mpi_w64']


def scene_of(g):
    import render_oracle as R
    head = {k[len('rgbnet_'):]: v for k, v in g.items() if k.startswith('rgbnet_')} or None
    mpi = int(g['mpi_depth']) if 'mpi_depth' in g else 0
    kw = dict(fast_color_thres=float(g['fast_color_thres']), voxel_size_ratio=float(g['voxel_size_ratio']),
              rgbnet=head, mpi_depth=mpi)
    if mpi:
        kw.update(act_shift=0.0, direct=True, viewbase_pe=0)
    else:
        direct = head is not None and g['rgbnet_0.weight'].shape[1] == 12 + 27
        kw.update(act_shift=float(g['act_shift']), voxel_size=float(g['voxel_size']), direct=direct, viewbase_pe=4)
    # the feature grid as the product stores it: a channels-last view
    k0 = g['k0'][0]
    k0_cl = np.ascontiguousarray(k0.transpose(1, 2, 3, 0)).transpose(3, 0, 1, 2)
    return R.Scene(g['xyz_min'], g['xyz_max'], g['density'], k0_cl, g['mask'], **kw)


def render_kwargs(g):
    if 'mpi_depth' in g:
        return dict(near=0, far=1, stepsize=float(g['stepsize']), bg=float(g['bg']))
    return dict(near=float(g['near']), far=float(g['far']), stepsize=float(g['stepsize']), bg=float(g['bg']))


def loss_weights(name):
    return (0.01, 0.1) if name == 'forward_coarse' else (0.001, 0.01)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('name', FIXTURES)
def test_helper_reproduces_the_reference_forward_and_backward(name, dtype, oracle):
    import render_oracle as R
    g = load_golden(name)
    sc = scene_of(g)
    assert sc.k0.strides[0] == 4                                        # reads the channels-last layout in place
    out = R.forward(sc, g['rays_o'], g['rays_d'], g['viewdirs'], dtype=dtype, **render_kwargs(g))
    assert np.array_equal(out['ray_id'], g['out_ray_id'])
    np.testing.assert_allclose(out['weights'], g['out_weights'], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(out['raw_alpha'], g['out_raw_alpha'], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(out['alphainv_last'], g['out_alphainv_last'], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(out['raw_rgb'], g['out_raw_rgb'], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(out['rgb_marched'], g['out_rgb_marched'], atol=1e-5)
    np.testing.assert_allclose(out['depth'], g['out_depth'], rtol=1e-5, atol=1e-4)
    assert out['feat'].shape == (out['weights'].shape[0], sc.k0.shape[0]) and out['pts'].shape == (out['weights'].shape[0], 3)
    w_ent, w_per = loss_weights(name)
    loss, grads = R.loss_and_grads(sc, out, g['target'], w_ent=w_ent, w_per=w_per)
    np.testing.assert_allclose(loss, float(g['loss']), rtol=1e-5)
    np.testing.assert_allclose(grads['grad_density'], g['grad_density'][0, 0], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(grads['grad_k0'], g['grad_k0'][0], rtol=1e-4, atol=1e-6)
    names = [k[len('grad_rgbnet_'):] for k in g if k.startswith('grad_rgbnet_')]
    assert sorted(names) == sorted(k[len('grad_rgbnet_'):] for k in grads if k.startswith('grad_rgbnet_'))
    for k in names:
        np.testing.assert_allclose(grads['grad_rgbnet_' + k], g['grad_rgbnet_' + k], rtol=1e-3, atol=1e-6)
    assert np.abs(grads['grad_k0']).max() > 0 and np.abs(grads['grad_density']).max() > 0
    assert grads['g_feat'].shape == out['feat'].shape
    if sc.head is not None:
        margin = R.relu_margin(sc, out)
        assert margin.shape == out['weights'].shape and (margin >= 0).all() and np.median(margin) > 1e-4


@pytest.mark.parametrize('name', ['forward_coarse', 'forward_fine', 'forward_fine_direct'])
def test_helper_hit_test_and_samples_match_the_reference(name, oracle):
    import render_oracle as R
    g = load_golden(name)
    sc = scene_of(g)
    rk = render_kwargs(g)
    hit = R.hit_coarse_geo(sc, g['rays_o'], g['rays_d'], rk['near'], rk['far'], rk['stepsize'])
    assert np.array_equal(hit, g['hit'])
    pts, ray_id, step_id = R._sample(sc, g['rays_o'], g['rays_d'], rk['near'], rk['far'], rk['stepsize'])
    assert np.array_equal(pts, g['sample_ray_pts'])
    assert np.array_equal(ray_id, g['sample_ray_id'])
    assert np.array_equal(step_id, g['sample_step_id'])


def test_helper_chunks_the_head_without_changing_a_gradient(oracle, monkeypatch):
    """The head runs in row chunks at full size: a chunk boundary inside the batch changes nothing beyond rounding
    (float64: the weight-gradient sums are split in two)."""
    import render_oracle as R
    g = load_golden('forward_fine_direct')
    sc = scene_of(g)
    outs = []
    for chunk in (R.HEAD_CHUNK, 7):
        monkeypatch.setattr(R, 'HEAD_CHUNK', chunk)
        out = R.forward(sc, g['rays_o'], g['rays_d'], g['viewdirs'], dtype=torch.float64, **render_kwargs(g))
        assert out['weights'].shape[0] > 7
        outs.append((out, R.loss_and_grads(sc, out, g['target'])[1]))
    (a, ga), (b, gb) = outs
    # (the BLAS blocks a float64 GEMM differently at 7 rows than at 1634: last-bit differences only)
    np.testing.assert_allclose(a['raw_rgb'], b['raw_rgb'], rtol=1e-13, atol=0)
    for k in ga:
        np.testing.assert_allclose(ga[k], gb[k], rtol=1e-6, atol=1e-12 * np.abs(gb[k]).max())
