"""Generate the tri-plane fixtures by RUNNING THE REFERENCE's own Python (lib/tri_dvgo.py), through
make_golden.import_reference() (a scratch copy with the oracle-backed natives), never in place.  Runs only where the
reference tree exists; the files it writes are committed, arrays only:

  triplane.npz           grid_sampler2D (lib/tri_dvgo.py:456-469, pure PyTorch: three F.grid_sample + cat / sum) and its
                         autograd backward on planes of different, non-square sizes (one with an axis of size 1), points
                         on the box corners, on texel centres and up to 5 % outside the box; both aggregations.
  forward_triplane.npz   DirectVoxGO.render (lib/tri_dvgo.py:688-809) on caller-supplied planes for a tiny scene, with the
                         loss of run.py:377-386 and its gradients w.r.t. the planes, the density grid and the MLP; both
                         aggregations (keys prefixed 'concat_' / 'sum_'; the scene and the rays are shared).

The reference class is constructed as it stands (its encoder is built and never called: `render` takes the planes).

Usage:  python tests/golden/make_golden_triplane.py
"""
import os
import shutil
import sys
from unittest import mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

KEYS = ('xy', 'yz', 'zx')


def import_tri(R):
    for missing in ('matplotlib', 'matplotlib.pyplot'):
        try:
            __import__(missing)
        except Exception:
            sys.modules[missing] = mock.MagicMock()
    import lib.tri_dvgo as tri
    return tri


def _model(tri, mn, mx, agg, nvox, **kw):
    torch.manual_seed(777)
    return tri.DirectVoxGO(mn, mx, num_voxels=nvox, num_voxels_base=nvox, alpha_init=1e-2, fast_color_thres=1e-4,
                           tri_aggregation=agg, n_resblocks=1, n_feats=8, **kw)


def gen_sampler(tri):
    rng = np.random.default_rng(1201)
    mn, mx = np.array([-1.0, -0.8, -0.6], np.float32), np.array([0.9, 1.1, 0.7], np.float32)
    C = 5
    sizes = {'xy': (6, 7), 'yz': (3, 9), 'zx': (8, 1)}
    planes = {k: rng.standard_normal((1, C, *hw)).astype(np.float32) for k, hw in sizes.items()}
    M = 400
    xyz = (rng.random((M, 3)) * (mx - mn) * 1.1 + mn - 0.05 * (mx - mn)).astype(np.float32)   # up to 5 % outside
    corners = np.array([[(mn, mx)[(i >> a) & 1][a] for a in range(3)] for i in range(8)], np.float32)
    xyz[:8] = corners
    # texel centres of plane xy (rows y, columns z) and of plane yz (rows x, columns y)
    for i in range(8, 20):
        xyz[i, 1] = mn[1] + (mx[1] - mn[1]) * (i % 6) / 5
        xyz[i, 2] = mn[2] + (mx[2] - mn[2]) * (i % 7) / 6
        xyz[i, 0] = mn[0] + (mx[0] - mn[0]) * (i % 3) / 2
    out = {'xyz_min': mn, 'xyz_max': mx, 'xyz': xyz}
    for k in KEYS:
        out['plane_' + k] = planes[k]
    for agg in ('concat', 'sum'):
        m = _model(tri, mn, mx, agg, 8 ** 3, rgbnet_dim=C, rgbnet_width=16)
        feats = {k: torch.from_numpy(v).clone().requires_grad_() for k, v in planes.items()}
        val = m.grid_sampler2D(torch.from_numpy(xyz), feats)
        go = rng.standard_normal(tuple(val.shape)).astype(np.float32)
        val.backward(torch.from_numpy(go))
        out[agg + '_out'] = val.detach().numpy()
        out[agg + '_gout'] = go
        for k in KEYS:
            out[f'{agg}_gplane_{k}'] = feats[k].grad.numpy()
    make_golden.save('triplane', **out)


def gen_forward(R, tri):
    rng = np.random.default_rng(1202)
    mn, mx = np.array([-1.05] * 3, np.float32), np.array([1.05] * 3, np.float32)
    C = 4
    sizes = {'xy': (9, 11), 'yz': (7, 10), 'zx': (12, 8)}
    planes = {k: (rng.standard_normal((1, C, *hw)) * 0.3).astype(np.float32) for k, hw in sizes.items()}
    ro, rd, vd = make_golden.lego_like_rays(R, rng, n_views=4, H=5, W=5, focal=5 * 1111.11 / 800 * 3.0, radius=3.0)
    ro = torch.cat([ro, torch.tensor([[3.0, 3.0, 3.0], [0.0, 0.0, 3.0], [0.1, 0.1, 0.2]])])
    rd = torch.cat([rd, torch.tensor([[1.0, 0.2, 0.1], [0.0, 1.0, 0.0], [0.4, -0.3, 0.2]])])
    vd = rd / rd.norm(dim=-1, keepdim=True)
    N = ro.shape[0]
    target = torch.from_numpy(rng.random((N, 3)).astype(np.float32))
    rk = dict(near=0.5, far=6.0, bg=1, stepsize=0.5, inverse_y=False, flip_x=False, flip_y=False, render_depth=True)
    out = dict(xyz_min=mn, xyz_max=mx, rays_o=ro, rays_d=rd, viewdirs=vd, target=target, near=rk['near'], far=rk['far'],
               bg=rk['bg'], stepsize=rk['stepsize'], rgbnet_dim=np.int64(C))
    for k in KEYS:
        out['plane_' + k] = planes[k]
    dens = None
    for agg in ('concat', 'sum'):
        m = _model(tri, mn, mx, agg, 16 ** 3, rgbnet_dim=C, rgbnet_depth=3, rgbnet_width=64, viewbase_pe=4, rgbnet_direct=False)
        ws = tuple(int(v) for v in m.world_size)
        with torch.no_grad():
            if dens is None:
                dens = make_golden.blob_density(ws, mn, mx, rng)
            m.density.copy_(torch.from_numpy(dens)[None, None])
            alpha = torch.nn.functional.max_pool3d(m.activate_density(m.density), 3, 1, 1)[0, 0]
            m.mask_cache.mask.copy_(alpha > m.fast_color_thres)
            for p in m.rgbnet.parameters():
                p.add_(torch.from_numpy((rng.standard_normal(tuple(p.shape)) * 0.05).astype(np.float32)))
        feats = {k: torch.from_numpy(v).clone().requires_grad_() for k, v in planes.items()}
        res = m.render(feats, ro, rd, vd, 0, **rk)
        loss = make_golden._loss(res, target, N)
        loss.backward()
        out.update(world_size=np.array(ws), density=m.density.detach().numpy().copy(), mask=m.mask_cache.mask.numpy().copy(),
                   fast_color_thres=np.float64(m.fast_color_thres))
        out[agg + '_loss'] = loss.detach()
        out[agg + '_grad_density'] = m.density.grad
        for k in KEYS:
            out[f'{agg}_grad_plane_{k}'] = feats[k].grad
        for k, v in res.items():
            out[f'{agg}_out_{k}'] = v
        for k, v in m.rgbnet.state_dict().items():
            out[f'{agg}_rgbnet_{k}'] = v
        for k, v in m.rgbnet.named_parameters():
            out[f'{agg}_grad_rgbnet_{k}'] = v.grad
    make_golden.save('forward_triplane', **out)


def main():
    R = make_golden.import_reference()
    try:
        tri = import_tri(R)
        gen_sampler(tri)
        gen_forward(R, tri)
    finally:
        shutil.rmtree(R.scratch, ignore_errors=True)


if __name__ == '__main__':
    main()
