"""Generate the LIIF plane-decoder fixtures by RUNNING THE REFERENCE's own Python (lib/tri_dvgo.py with
implicit_voxel_feat=True, liif=True), through make_golden.import_reference() as make_golden_triplane.py does.  Runs only
where the reference tree exists; the files it writes are committed, arrays only.  The reference model is put in eval()
mode: the Interp_MLPs' dropout is off.

  liif.npz           liif_interpolate (lib/tri_dvgo.py:481-565) and its autograd gradients w.r.t. the planes and the
                     Interp_MLP parameters, for {concat, sum} x cell_decode {1, 0} x local_ensemble {1, 0} (keys prefixed
                     '<agg>_c<cell>_e<ens>_'; the output gradient '<agg>_gout' is shared by an aggregation's cases): C = 5,
                     planes (6,7), (3,9), (8,1), a non-cubic world_size, 400 points that include the box corners and
                     points up to 5 % outside.  Values: the float32 run.  Gradients: the same reference code on float64
                     copies of the model and the inputs (same texels: its values are checked against the float32 run's).  The MLP state_dicts are stored per cell_decode
                     under the reference's key names ('c<cell>_sd_interp_xy.model.0.weight', ...).
  forward_liif.npz   DirectVoxGO.render (lib/tri_dvgo.py:688-809) with the loss of run.py:377-386 and its gradients w.r.t.
                     the planes, the density grid, the Interp_MLPs and rgbnet, on the scene, planes and rays of
                     forward_triplane.npz (read from that file, not stored again).  Case 'sum': tri_aggregation='sum',
                     cell_decode=True; case 'pe': 'concat' with posbase_pe=2, cat_posemb=True.

Nearest-texel picks are discontinuous in the position, so every point of liif.npz is checked against the float32 oracle
(tests/liif_oracle.py) with the reference's own MLPs: a point whose decoded value differs by more than the fixture
tolerance (rtol 1e-5 / atol 1e-6) is replaced by a fresh one, and more than 1 % replaced points is an error.

Usage:  python tests/golden/make_golden_liif.py
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
import liif_oracle as LO  # noqa: E402

KEYS = T.KEYS
INTERP = ('interp_xy', 'interp_yz', 'interp_zx')


def _model(tri, mn, mx, agg, nvox, **kw):
    m = T._model(tri, mn, mx, agg, nvox, implicit_voxel_feat=True, liif=True, feat_unfold=False, **kw)
    return m.eval()


def _oracle_values(m, planes, xyz, mn, mx, agg, cell, ens):
    """the reference's float32 MLPs on the oracle's rows, blended by the oracle"""
    ws = [int(v) for v in m.world_size]
    inp, wgt = LO.rows(planes, xyz, mn, mx, ws, cell, ens)
    with torch.no_grad():
        pred = np.stack([m.interp[k](torch.from_numpy(inp[s])).numpy() for s, k in enumerate(KEYS)])
    return LO.blend(pred, wgt, agg)[0]


def gen_decoder(tri):
    rng = np.random.default_rng(1301)
    mn, mx = np.array([-1.0, -0.8, -0.6], np.float32), np.array([0.9, 1.1, 0.7], np.float32)
    C, M = 5, 400
    sizes = {'xy': (6, 7), 'yz': (3, 9), 'zx': (8, 1)}
    planes = {k: rng.standard_normal((1, C, *hw)).astype(np.float32) for k, hw in sizes.items()}

    def fresh(n):
        return (rng.random((n, 3)) * (mx - mn) * 1.1 + mn - 0.05 * (mx - mn)).astype(np.float32)   # up to 5 % outside

    xyz = fresh(M)
    xyz[:8] = np.array([[(mn, mx)[(i >> a) & 1][a] for a in range(3)] for i in range(8)], np.float32)
    cases = [(agg, cell, ens) for agg in ('concat', 'sum') for cell in (True, False) for ens in (True, False)]
    kw = dict(rgbnet_dim=C, rgbnet_width=16, interp_width=8, interp_depth=3)
    replaced = 0
    for _ in range(4):                      # settle the points first: every case must agree with the oracle on every point
        bad = np.zeros(M, bool)
        for agg, cell, ens in cases:
            m = _model(tri, mn, mx, agg, 1600, cell_decode=cell, local_ensemble=ens, **kw)
            with torch.no_grad():
                ref = m.liif_interpolate(torch.from_numpy(xyz), {k: torch.from_numpy(v) for k, v in planes.items()}).numpy()
            ora = _oracle_values(m, planes, xyz, mn, mx, agg, cell, ens)
            bad |= (np.abs(ora - ref) > 1e-6 + 1e-5 * np.abs(ref)).any(1)
        if not bad.any():
            break
        assert not bad[:8].any(), 'a box corner disagrees with the oracle'
        replaced += int(bad.sum())
        xyz[bad] = fresh(int(bad.sum()))
    else:
        raise RuntimeError('points keep disagreeing with the oracle')
    print('replaced points:', replaced)
    assert replaced <= M // 100, replaced
    out = {'xyz_min': mn, 'xyz_max': mx, 'xyz': xyz}
    for k in KEYS:
        out['plane_' + k] = planes[k]
    for agg, cell, ens in cases:
        m = _model(tri, mn, mx, agg, 1600, cell_decode=cell, local_ensemble=ens, **kw)
        ws = tuple(int(v) for v in m.world_size)
        assert len(set(ws)) > 1, ws
        out['world_size'] = np.array(ws)
        p = f'{agg}_c{int(cell)}_e{int(ens)}_'
        with torch.no_grad():
            val = m.liif_interpolate(torch.from_numpy(xyz), {k: torch.from_numpy(v) for k, v in planes.items()})
        out[p + 'out'] = val.numpy()
        if agg + '_gout' not in out:          # one output gradient per aggregation, shared by its four cases
            out[agg + '_gout'] = rng.standard_normal(tuple(val.shape)).astype(np.float32)
        # the gradients: the same code on float64 copies of the same numbers.  In float32 a weight gradient is a sum over
        # up to 3200 rows whose own rounding (a few 2^-24 of the sum of its |terms|) exceeds the fixture tolerance where
        # the terms cancel; the float64 run takes the same texels (its values agree with the float32 run's below).
        m64 = copy.deepcopy(m).double()
        feats = {k: torch.from_numpy(v).double().requires_grad_() for k, v in planes.items()}
        val64 = m64.liif_interpolate(torch.from_numpy(xyz).double(), feats)
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
    make_golden.save('liif', **out)


def gen_forward(tri):
    rng = np.random.default_rng(1302)
    g = np.load(os.path.join(HERE, 'forward_triplane.npz'))
    mn, mx = g['xyz_min'], g['xyz_max']
    C = int(g['rgbnet_dim'])
    ro, rd, vd, target = (torch.from_numpy(g[k]) for k in ('rays_o', 'rays_d', 'viewdirs', 'target'))
    N = ro.shape[0]
    rk = dict(near=float(g['near']), far=float(g['far']), bg=int(g['bg']), stepsize=float(g['stepsize']), inverse_y=False,
              flip_x=False, flip_y=False, render_depth=True)
    out = {}
    for tag, agg, extra in (('sum', 'sum', {}), ('pe', 'concat', dict(posbase_pe=2, cat_posemb=True))):
        m = _model(tri, mn, mx, agg, 16 ** 3, rgbnet_dim=C, rgbnet_depth=3, rgbnet_width=64, viewbase_pe=4, rgbnet_direct=False,
                   cell_decode=True, local_ensemble=True, interp_width=16, interp_depth=3, **extra)
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
        p = tag + '_'
        out[p + 'loss'] = loss.detach()
        out[p + 'grad_density'] = m.density.grad
        for k in KEYS:
            out[f'{p}grad_plane_{k}'] = feats[k].grad
        for k, v in res.items():
            out[f'{p}out_{k}'] = v
        for k, v in m.state_dict().items():
            if k.startswith(('rgbnet.', 'interp_')):
                out[f'{p}sd_{k}'] = v
        for k, v in m.named_parameters():
            if k.startswith(('rgbnet.', 'interp_xy.', 'interp_yz.')):
                out[f'{p}grad_{k}'] = v.grad
            elif k.startswith('interp_zx.'):
                assert v.grad is None
    make_golden.save('forward_liif', **out)


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
