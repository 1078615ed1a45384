"""Generate the bilinear plane-decoder fixtures by RUNNING THE REFERENCE's own Python (lib/tri_dvgo.py with
implicit_voxel_feat=True, liif=False), through make_golden.import_reference() as make_golden_liif.py does.  Runs only
where the reference tree exists; the files it writes are committed, arrays only.  The reference model is put in eval()
mode: the Interp_MLPs' dropout is off.

  interp.npz           interpolate (lib/tri_dvgo.py:568-607) and its autograd gradients w.r.t. the planes and the Interp_MLP
                       parameters, for {concat, sum} x cell_decode {1, 0} (keys prefixed '<agg>_c<cell>_'; the output gradient
                       '<agg>_gout' is shared by an aggregation's cases): C = 5, posbase_pe = 2, planes (6,7), (3,9), (8,1), a
                       non-cubic world_size, 400 points that include the box corners, texel centres and points up to 5 %
                       outside.  Values: the float32 run.  Gradients: the same reference code on float64 copies of the model
                       and the inputs.  The MLP state_dicts are stored per cell_decode under the reference's key names
                       ('c<cell>_sd_interp_xy.model.0.weight', ...).
  forward_interp.npz   DirectVoxGO.render (lib/tri_dvgo.py:688-809) with the loss of run.py:377-386 and its gradients w.r.t.
                       the planes, the density grid, the Interp_MLPs and rgbnet, on the scene, planes and rays of
                       forward_triplane.npz (read from that file, not stored again): tri_aggregation='sum', cell_decode=True,
                       posbase_pe=2, cat_posemb=True.  'ref_keys': the reference model's state_dict key set.

The decoder is continuous in the position, so no point is replaced: every point of interp.npz must agree with the oracle
(tests/interp_oracle.py) run through the reference's own MLPs at rtol 1e-5 / atol 1e-6, or the generator fails.

Usage:  python tests/golden/make_golden_interp.py
"""
import copy
import os
import shutil
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402
import make_golden_triplane as T  # noqa: E402
import interp_oracle as IO  # noqa: E402

KEYS = T.KEYS
INTERP = ('interp_xy', 'interp_yz', 'interp_zx')
P = 2


def _model(tri, mn, mx, agg, nvox, **kw):
    m = T._model(tri, mn, mx, agg, nvox, implicit_voxel_feat=True, liif=False, feat_unfold=False, posbase_pe=P, **kw)
    return m.eval()


def _oracle_values(m, planes, xyz, mn, mx, agg, cell):
    """the reference's float32 MLPs on the oracle's float32 rows"""
    ws = [int(v) for v in m.world_size]
    inp = IO.rows(planes, xyz, mn, mx, ws, P, cell)
    with torch.no_grad():
        pred = [m.interp[k](torch.from_numpy(inp[s])).numpy() for s, k in enumerate(KEYS)]
    return np.concatenate(pred, 1) if agg == 'concat' else (pred[0] + pred[1]) + pred[2]


def gen_decoder(tri):
    rng = np.random.default_rng(1401)
    mn, mx = np.array([-1.0, -0.8, -0.6], np.float32), np.array([0.9, 1.1, 0.7], np.float32)
    C, M = 5, 400
    sizes = {'xy': (6, 7), 'yz': (3, 9), 'zx': (8, 1)}
    planes = {k: rng.standard_normal((1, C, *hw)).astype(np.float32) for k, hw in sizes.items()}
    xyz = (rng.random((M, 3)) * (mx - mn) * 1.1 + mn - 0.05 * (mx - mn)).astype(np.float32)   # up to 5 % outside
    xyz[:8] = np.array([[(mn, mx)[(i >> a) & 1][a] for a in range(3)] for i in range(8)], np.float32)
    for i in range(8, 20):          # texel centres of plane xy (rows y, columns z) and of plane yz (rows x, columns y)
        xyz[i, 1] = mn[1] + (mx[1] - mn[1]) * (i % 6) / 5
        xyz[i, 2] = mn[2] + (mx[2] - mn[2]) * (i % 7) / 6
        xyz[i, 0] = mn[0] + (mx[0] - mn[0]) * (i % 3) / 2
    cases = [(agg, cell) for agg in ('concat', 'sum') for cell in (True, False)]
    kw = dict(rgbnet_dim=C, rgbnet_width=16, interp_width=8, interp_depth=3)
    out = {'xyz_min': mn, 'xyz_max': mx, 'xyz': xyz, 'posbase_pe': np.array(P)}
    for k in KEYS:
        out['plane_' + k] = planes[k]
    for agg, cell in cases:
        m = _model(tri, mn, mx, agg, 1600, cell_decode=cell, **kw)
        ws = tuple(int(v) for v in m.world_size)
        assert len(set(ws)) > 1, ws
        out['world_size'] = np.array(ws)
        p = f'{agg}_c{int(cell)}_'
        with torch.no_grad():
            val = m.interpolate(torch.from_numpy(xyz), {k: torch.from_numpy(v) for k, v in planes.items()})
        out[p + 'out'] = val.numpy()
        ora = _oracle_values(m, planes, xyz, mn, mx, agg, cell)
        print(p, 'worst |oracle - reference|', float(np.abs(ora - out[p + 'out']).max()))
        np.testing.assert_allclose(ora, out[p + 'out'], rtol=1e-5, atol=1e-6)          # every point, none replaced
        if agg + '_gout' not in out:          # one output gradient per aggregation, shared by its cases
            out[agg + '_gout'] = rng.standard_normal(tuple(val.shape)).astype(np.float32)
        # the gradients: the same code on float64 copies of the same numbers (make_golden_liif.py has the reason)
        m64 = copy.deepcopy(m).double()
        feats = {k: torch.from_numpy(v).double().requires_grad_() for k, v in planes.items()}
        val64 = m64.interpolate(torch.from_numpy(xyz).double(), feats)
        np.testing.assert_allclose(val64.detach().numpy(), out[p + 'out'], rtol=1e-5, atol=1e-6)
        val64.backward(torch.from_numpy(out[agg + '_gout']).double())
        for k in KEYS:
            out[f'{p}gplane_{k}'] = feats[k].grad.numpy().astype(np.float32)
        for net in INTERP:
            for k, v in getattr(m, net).state_dict().items():
                key = f'c{int(cell)}_sd_{net}.{k}'
                assert key not in out or np.array_equal(out[key], v.numpy())      # one seed: the same MLPs in every case
                out[key] = v.numpy().copy()
            for k, v in getattr(m64, net).named_parameters():
                assert (v.grad is None) == (net == 'interp_zx')
                if v.grad is not None:
                    out[f'{p}g_{net}.{k}'] = v.grad.numpy().astype(np.float32)
    make_golden.save('interp', **out)


def gen_forward(tri):
    rng = np.random.default_rng(1402)
    g = np.load(os.path.join(HERE, 'forward_triplane.npz'))
    mn, mx = g['xyz_min'], g['xyz_max']
    C = int(g['rgbnet_dim'])
    ro, rd, vd, target = (torch.from_numpy(g[k]) for k in ('rays_o', 'rays_d', 'viewdirs', 'target'))
    N = ro.shape[0]
    rk = dict(near=float(g['near']), far=float(g['far']), bg=int(g['bg']), stepsize=float(g['stepsize']), inverse_y=False,
              flip_x=False, flip_y=False, render_depth=True)
    out = {}
    m = _model(tri, mn, mx, 'sum', 16 ** 3, rgbnet_dim=C, rgbnet_depth=3, rgbnet_width=64, viewbase_pe=4, rgbnet_direct=False,
               cell_decode=True, cat_posemb=True, interp_width=16, interp_depth=3)
    assert tuple(int(v) for v in m.world_size) == tuple(g['world_size'])
    with torch.no_grad():
        m.density.copy_(torch.from_numpy(g['density']))
        m.mask_cache.mask.copy_(torch.from_numpy(g['mask']))
        for p in m.rgbnet.parameters():
            p.add_(torch.from_numpy((rng.standard_normal(tuple(p.shape)) * 0.05).astype(np.float32)))
    feats = {k: torch.from_numpy(g['plane_' + k]).clone().requires_grad_() for k in KEYS}
    res = m.render(feats, ro, rd, vd, 0, **rk)
    loss = make_golden._loss(res, target, N)
    loss.backward()
    out['loss'] = loss.detach()
    out['grad_density'] = m.density.grad
    for k in KEYS:
        out[f'grad_plane_{k}'] = feats[k].grad
    for k, v in res.items():
        out[f'out_{k}'] = v
    out['ref_keys'] = np.array(sorted(m.state_dict().keys()))
    for k, v in m.state_dict().items():
        if k.startswith(('rgbnet.', 'interp_')):
            out[f'sd_{k}'] = v
    for k, v in m.named_parameters():
        if k.startswith(('rgbnet.', 'interp_xy.', 'interp_yz.')):
            out[f'grad_{k}'] = v.grad
        elif k.startswith('interp_zx.'):
            assert v.grad is None
    make_golden.save('forward_interp', **out)


def main():
    R = make_golden.import_reference()
    try:
        tri = T.import_tri(R)
        gen_decoder(tri)
        gen_forward(tri)
    finally:
        shutil.rmtree(R.scratch, ignore_errors=True)


if __name__ == '__main__':
    main()
