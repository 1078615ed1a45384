"""Host side of the fused march's ray gradient (no GPU):

  oracle against autograd   tests/march_raygrad_oracle.py's A and B per ray against torch float64 autograd of a direct
                            restatement -- render -> (rgb_marched ** 2).sum() -> gradient in rays_o and rays_d with the
                            stop-gradients of INTEGRATION.md section 7 -- on records the CPU oracle of the march produced
  header and validation     include/dvgo_hip.h declares dvgo_march_ray_bwd, _lib types it, and its validation codes come
                            back without a device
  attribute                 DirectVoxGO.fused_raygrad: False on a fresh model, not in get_kwargs(), not in a checkpoint

The restatement.  The oracle's inputs are the kernel's float32 intermediates (position, per-axis weights, exp_d, 1 + exp_d,
alpha, 1 - alpha, T, w = T alpha, alphainv_last: the records, and what `raygrad_oracle.inputs32` restates); a float64
re-evaluation of them from the rays differs from those values by float32 roundings, 1e-7, which is no test of a derivative at
1e-10.  So every such intermediate enters the graph as `value + (expr - expr.detach())`: the float32 value the oracle reads,
with the derivative of the expression that forms it (the clamp min(exp_d, 1e10) of K10 included).  The chain rule, the suffix
sums over a ray, the signs and pairings of the corner products, the scale, lam and both per-ray sums are autograd's.
"""
import ctypes

import numpy as np
import pytest
import torch

import march_cases as C
import march_oracle as M
import march_raygrad_oracle as MR
import raygrad_oracle as RG

_F = np.float32
BG = 1.0


def _st(value, expr):
    return torch.as_tensor(value, dtype=torch.float64) + (expr - expr.detach())


def _trilinear(grid, I, w_lo, w_hi):
    """grid [C,X,Y,Z] float64 tensor -> [E,C]; cell and in-range flags fixed (I), weights [E,3] each"""
    ijk0, inb = torch.from_numpy(I.ijk0), torch.from_numpy(I.inb)
    out = torch.zeros(ijk0.shape[0], grid.shape[0], dtype=torch.float64)
    for n in range(8):
        b = ((n >> 2) & 1, (n >> 1) & 1, n & 1)
        idx = [(ijk0[:, a] + b[a]).clamp(0, grid.shape[1 + a] - 1) for a in range(3)]
        v = grid[:, idx[0], idx[1], idx[2]].t()
        w = [(w_hi if b[a] else w_lo)[:, a] for a in range(3)]
        out = out + torch.where(inb[:, n, None], ((w[2] * w[1]) * w[0])[:, None] * v, torch.zeros_like(v))
    return out


def _restate(sc, q, t_min, k0, keep):
    """-> (grad_o, grad_d by autograd [N,3]; the upstream gradients gw [E], g_last [N], gfeat [E,C] of the same graph, numpy)
    `keep` [N]: rays that enter the loss (FINE_EXCLUDED says why the others do not)."""
    Rc = q.R
    o32, d32 = sc.arrays()
    N, E = o32.shape[0], Rc.ray.shape[0]
    o = torch.tensor(o32, dtype=torch.float64, requires_grad=True)
    d = torch.tensor(d32, dtype=torch.float64, requires_grad=True)
    dirs = (d32 / np.sqrt((d32.astype(np.float64) ** 2).sum(-1, keepdims=True))).astype(np.float32)
    p32 = MR.record_positions(Rc, q.start, dirs, sc.stepdist)
    dims = sc.density.shape
    I = RG.inputs32(p32, sc.xyz_min, sc.xyz_max, dims)
    lam, _ = MR.lam_reference(Rc, t_min, d32, sc.stepdist)
    ray = torch.from_numpy(Rc.ray)
    pts = _st(p32, o[ray] + d[ray] * torch.from_numpy(lam)[:, None])
    mn, mx = (torch.tensor(a.astype(np.float64)) for a in (sc.xyz_min, sc.xyz_max))
    g = (pts - mn) / (mx - mn) * (torch.tensor(dims, dtype=torch.float64) - 1)
    dg = g - g.detach()
    w_lo, w_hi = torch.from_numpy(I.w[:, :, 0].astype(np.float64)) - dg, torch.from_numpy(I.w[:, :, 1].astype(np.float64)) + dg
    dens = _trilinear(torch.tensor(sc.density[None].astype(np.float64)), I, w_lo, w_hi)[:, 0]
    e32 = Rc.exp_d.astype(np.float64)
    e = torch.from_numpy(e32) + torch.from_numpy(np.minimum(e32, 1e10)) * (dens - dens.detach())
    x = torch.from_numpy((_F(1) + Rc.exp_d).astype(np.float64)) + (e - e.detach())
    alpha = _st(Rc.alpha.astype(np.float64), 1 - x ** (-float(_F(sc.interval))))
    f = _st((_F(1) - Rc.alpha).astype(np.float64) + 1e-10, -alpha)
    logf = torch.log(f) - torch.log(f).detach()
    feat = _trilinear(torch.tensor(k0.astype(np.float64)), I, w_lo, w_hi)
    rgb = torch.sigmoid(feat[:, :3])
    marched = []
    w_all = []
    for r in range(N):
        a, b = int(Rc.first[r]), int(Rc.first[r + 1])
        L = torch.cumsum(logf[a:b], 0)
        Eb = torch.exp(torch.cat([torch.zeros(1, dtype=torch.float64), L[:-1]])) if b > a else logf[a:b]
        w = torch.from_numpy(Rc.w[a:b].astype(np.float64)) * Eb + torch.from_numpy(Rc.T[a:b].astype(np.float64)) * (alpha[a:b] - alpha[a:b].detach())
        last = float(q.last[r]) * (torch.exp(L[-1]) if b > a else torch.ones((), dtype=torch.float64))
        fl = torch.from_numpy(Rc.flag[a:b])
        w_all.append(w)
        marched.append((torch.where(fl, w, torch.zeros_like(w))[:, None] * rgb[a:b]).sum(0) + last * BG)
    marched = torch.stack(marched)
    loss = (marched[torch.from_numpy(keep)] ** 2).sum()
    go, gd = torch.autograd.grad(loss, (o, d))
    with torch.no_grad():
        gm = 2 * marched * torch.from_numpy(keep)[:, None]                       # d loss / d rgb_marched
        fl = torch.from_numpy(Rc.flag)
        gw = torch.where(fl, (gm[ray] * rgb).sum(-1), torch.zeros(E, dtype=torch.float64))
        g_last = gm.sum(-1) * BG
        w = torch.cat(w_all) if w_all else torch.zeros(0, dtype=torch.float64)
        gfeat = torch.zeros_like(feat)
        gfeat[:, :3] = torch.where(fl[:, None], gm[ray] * w[:, None] * rgb * (1 - rgb), torch.zeros_like(rgb))
    return go.numpy(), gd.numpy(), gw.numpy(), g_last.numpy(), gfeat.numpy()


def _random_scene():
    """9^3 lattice, random density around the activation's knee, tilted rays through the box from outside"""
    rng = np.random.default_rng(5)
    sc = C.Scene('rand9', 9, 1e-2, 1e-4, 12)
    sc.density[:] = rng.normal(2.0, 4.0, sc.density.shape).astype(np.float32)
    for _ in range(12):
        a = rng.uniform(0.5, 7.5, 3) * C.H
        dirn = rng.standard_normal(3)
        dirn *= rng.uniform(0.5, 2.0) / np.linalg.norm(dirn)
        sc.ray(tuple(a - 0.4 * dirn / np.linalg.norm(dirn)), tuple(dirn))
    sc.near, sc.far = 0.05, 1.0
    return sc


# rays of the edge-case table that the RESTATEMENT cannot differentiate, each with what excludes it (march_cases.fine_scene).
# The oracle itself is finite there (p = (1 + inf)^-1.5 == 0 gives g_d == 0, as the kernel's exp2(-inf) does).
FINE_EXCLUDED = {23: 'row exp=inf: exp_d == inf, so value + (expr - expr.detach()) is inf - inf in torch'}


@pytest.mark.parametrize('name', ['fine129', 'rand9'])
def test_oracle_equals_autograd_of_a_direct_restatement(name, oracle):
    sc = C.fine_scene() if name == 'fine129' else _random_scene()
    q = C.cpu_forward(sc, oracle)
    Rc = q.R
    o32, d32 = sc.arrays()
    N = o32.shape[0]
    t_min = oracle.sample_pts_on_rays(o32, d32, sc.xyz_min, sc.xyz_max, sc.near, sc.far, float(_F(sc.stepdist)))[5]
    k0 = (0.3 * np.random.default_rng(7).standard_normal((sc.C, *sc.density.shape))).astype(np.float32)
    inf_rays = sorted(set(Rc.ray[~np.isfinite(Rc.exp_d)].tolist()))
    if name == 'fine129':
        assert inf_rays == sorted(FINE_EXCLUDED) and Rc.ray.shape[0] > 1500 and int(Rc.n.max()) == 256
    else:
        assert inf_rays == [] and Rc.ray.shape[0] > 60
    keep = np.ones(N, bool)
    keep[inf_rays] = False
    go, gd, gw, g_last, gfeat = _restate(sc, q, t_min, k0, keep)
    dirs = (d32 / np.sqrt((d32.astype(np.float64) ** 2).sum(-1, keepdims=True))).astype(np.float32)
    G = MR.reference(Rc, q.last, gw, g_last, float(_F(sc.interval)), q.start, dirs, sc.stepdist, sc.xyz_min, sc.xyz_max,
                     sc.density, k0, gfeat, t_min, d32)
    assert float(np.abs(G.A[keep]).max()) > 1e-3 and float(np.abs(G.B[keep]).max()) > 1e-3
    for what, got, ref, mag in (('A', go, G.A, G.magA), ('B', gd, G.B, G.magB)):
        err = np.abs(got - ref)[keep]
        tol = 1e-10 * mag[keep]
        assert np.all(err <= tol), (name, what, float((err - tol).max()), np.argwhere(err > tol)[:5].tolist())
    assert np.all(G.A[Rc.n == 0] == 0) and np.all(go[Rc.n == 0] == 0)
    # the bound is positive wherever something contributes, and a ray without upstream gradient contributes nothing
    assert np.all(G.boundA[keep & (Rc.n > 0)] > 0)


def test_bound_scales_with_the_terms_and_a_wrong_evaluation_falls_outside(oracle):
    """`check` accepts the reference itself rounded to float32, rejects a sign flip of grad_d and a dropped record, and
    refuses an exclusion list that is not exactly the rays without a finite reference."""
    sc = C.fine_scene()
    q = C.cpu_forward(sc, oracle)
    Rc = q.R
    o32, d32 = sc.arrays()
    t_min = oracle.sample_pts_on_rays(o32, d32, sc.xyz_min, sc.xyz_max, sc.near, sc.far, float(_F(sc.stepdist)))[5]
    rng = np.random.default_rng(11)
    k0 = (0.3 * rng.standard_normal((sc.C, *sc.density.shape))).astype(np.float32)
    gw = np.where(Rc.flag, rng.standard_normal(Rc.ray.shape[0]), 0).astype(np.float32)
    g_last = rng.standard_normal(Rc.n.shape[0]).astype(np.float32)
    gfeat = np.where(Rc.flag[:, None], rng.standard_normal((Rc.ray.shape[0], sc.C)), 0).astype(np.float32)
    dirs = (d32 / np.sqrt((d32.astype(np.float64) ** 2).sum(-1, keepdims=True))).astype(np.float32)
    G = MR.reference(Rc, q.last, gw, g_last, float(_F(sc.interval)), q.start, dirs, sc.stepdist, sc.xyz_min, sc.xyz_max,
                     sc.density, k0, gfeat, t_min, d32)
    excluded = []                     # every ray of the table has a finite reference (exp_d == inf: p == 0, g_d == 0)
    assert G.finite.all() and np.isfinite(G.boundA).all() and np.isfinite(G.boundB).all()
    A, Bv = np.nan_to_num(G.A).astype(np.float32), np.nan_to_num(G.B).astype(np.float32)
    assert MR.check(G, A, Bv, excluded) <= 1.0
    with pytest.raises(AssertionError, match='finite reference'):
        MR.check(G, A, Bv, [23])
    with pytest.raises(AssertionError, match='grad_d'):
        MR.check(G, A, -Bv, excluded)
    r = int(np.argmax(np.where(G.finite, G.n, 0)))                          # the longest ray with a reference ...
    worst = np.argmax(np.where(Rc.ray == r, np.abs(G.ref_p[:, 0]), 0))      # ... without its largest term
    A2 = A.copy()
    A2[r] -= G.ref_p[worst].astype(np.float32)
    with pytest.raises(AssertionError, match='grad_o'):
        MR.check(G, A2, Bv, excluded)


# ------------------------------------------------------------------------------------------ header, validation
def test_header_declares_the_entry_and_lib_types_it():
    from directvoxgo_amd import _lib, build
    build.build(verbose=False)
    with open(_lib.HEADER_PATH) as f:
        decl = _lib.declarations(f.read())
    restype, argtypes = decl['dvgo_march_ray_bwd']
    P, i, q, fl = _lib._Pointer, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert restype is ctypes.c_int
    assert argtypes == [P, P, P, P, q, P, q, P, P, fl, P, P, P, fl, P, P, fl, fl, P, i, i, i, P, i, q, q, q, q, P, P, P, P, P, P]
    fn = _lib.lib().dvgo_march_ray_bwd
    assert fn.argtypes == argtypes and _lib.ABI_VERSION == _lib.lib().dvgo_abi_version() == 11


def _args(n_rays=4, stepdist=0.5, C=12, X=4, null=(), rec_stride=16, cum=False):
    """the argument list with every pointer a non-null value that is never dereferenced (the calls return on validation)"""
    one = ctypes.c_void_p(16)
    names = ['rec2', 'n2', 'n_steps', 'cum', 'rec_stride', 'off3', 'n_rays', 'rays_start', 'rays_dir', 'stepdist', 'xyz_min',
             'xyz_max', 'last', 'interval', 'rays_o', 'rays_d', 'near', 'far', 'density', 'X', 'Y', 'Z', 'k0', 'C', 'sC', 'sX', 'sY',
             'sZ', 'grad_weights', 'grad_last', 'grad_feat', 'grad_o', 'grad_d', 'stream']
    vals = dict.fromkeys(names, one)
    vals.update(cum=one if cum else None, rec_stride=rec_stride, n_rays=n_rays, stepdist=stepdist, interval=0.5, near=0.0, far=1.0,
                X=X, Y=4, Z=4, C=C, sC=1, sX=16 * C, sY=4 * C, sZ=C, stream=None)
    for k in null:
        vals[k] = None
    return [vals[k] for k in names]


def test_validation_answers_before_any_launch():
    from directvoxgo_amd import _lib
    fn = _lib.lib().dvgo_march_ray_bwd
    assert fn(*_args(n_rays=-1)) == -1
    assert fn(*_args(C=-1)) == -1
    assert fn(*_args(X=0)) == -1
    assert fn(*_args(stepdist=0.0)) == -1
    assert fn(*_args(stepdist=-255.0)) == -1                     # NDC spacing is not differentiated
    assert fn(*_args(n_rays=0)) == 0
    assert fn(*_args(n_rays=0, null=('rec2', 'grad_o', 'density'))) == 0
    for k in ('rec2', 'n2', 'n_steps', 'off3', 'rays_start', 'rays_dir', 'xyz_min', 'xyz_max', 'last', 'rays_o', 'rays_d', 'density',
              'grad_o', 'grad_d'):
        assert fn(*_args(null=(k,))) == -1, k                    # each required pointer is looked at
    assert fn(*_args(null=('k0',))) == -1                        # a feature term without a feature grid
    assert fn(*_args(rec_stride=0)) == -1                        # neither layout
    assert fn(*_args(n_rays=1 << 25)) == -2                      # n_rays * 64 == 2^31
    assert fn(*_args(n_rays=1 << 25, null=('grad_last', 'grad_feat', 'grad_weights', 'k0'), cum=True, rec_stride=0)) == -2
    with pytest.raises(RuntimeError, match='invalid argument'):
        _lib.call('dvgo_march_ray_bwd', *_args(stepdist=0.0))


# ------------------------------------------------------------------------------------------ the model's switch
def test_fused_raygrad_is_a_switch_of_the_process_not_of_the_model(tmp_path):
    from directvoxgo_amd import checkpoint
    from directvoxgo_amd.dvgo import DirectVoxGO
    m = DirectVoxGO([-1, -1, -1], [1, 1, 1], num_voxels=8 ** 3, num_voxels_base=8 ** 3, alpha_init=1e-2)
    assert DirectVoxGO.fused_raygrad is False and m.fused_raygrad is False and 'fused_raygrad' not in m.__dict__
    assert 'fused_raygrad' not in m.get_kwargs() and not any('fused_raygrad' in k for k in m.state_dict())
    m.fused_raygrad = True
    path = str(tmp_path / 'ckpt.tar')
    checkpoint.save_checkpoint(path, m, None, 3)
    ckpt = checkpoint.safe_load(path)
    assert 'fused_raygrad' not in str(sorted(ckpt)) and 'fused_raygrad' not in ckpt['model_kwargs']
    assert not any('fused_raygrad' in k for k in ckpt['model_state_dict'])
    m2 = checkpoint.load_model(DirectVoxGO, path)
    assert m2.fused_raygrad is False and 'fused_raygrad' not in m2.__dict__


def test_refine_poses_fused_needs_a_fused_model():
    from directvoxgo_amd.dvgo import DirectVoxGO
    from directvoxgo_amd.pose import CameraRefiner, refine_poses
    from directvoxgo_amd.train import FINE_TRAIN
    m = DirectVoxGO([-1, -1, -1], [1, 1, 1], num_voxels=8 ** 3, num_voxels_base=8 ** 3, alpha_init=1e-2, fused=False)
    pose = torch.eye(4)[None, :3]
    K = np.array([[10.0, 0, 2], [0, 10.0, 2], [0, 0, 1]], np.float32)
    ref = CameraRefiner(pose, [[4, 4]], [K])
    with pytest.raises(ValueError, match='fused'):
        refine_poses(m, ref, torch.zeros(1, 4, 4, 3), FINE_TRAIN, dict(near=0.1, far=1.0, stepsize=0.5, bg=1), 1, 8, 1e-3, fused=True)
    assert 'fused_raygrad' not in m.__dict__
