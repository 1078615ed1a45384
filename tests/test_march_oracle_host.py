"""Host side of tests/march_oracle.py and tests/march_cases.py (no GPU): the float64 chain is pinned by torch float64
autograd, a correct float32 evaluation in either summation order stays inside the derived bounds with no record left out,
wrong evaluations fall outside, and every row of the edge-case table hits its edge on the CPU oracle alone."""
import numpy as np
import pytest
import torch

import march_cases as C
import march_oracle as M

_F = np.float32


class _Rec64:
    """Records with float64 fields (the formulas are pinned free of float32 rounding)"""


def _ragged(rng, n_rays, n_max, amax=0.9, opaque=0.3, thres=0.0):
    rays = []
    for r in range(n_rays):
        n = int(rng.integers(1, n_max + 1))
        a = (rng.uniform(0, 1, n) ** 3 * (amax if r % 2 else 0.02)).astype(np.float32)      # (every other ray: thin, runs long)
        if rng.uniform() < opaque:
            a[-1] = 1.0 if rng.uniform() < 0.5 else _F(1) - _F(2.0 ** -24)
        rays.append(a)
    return M.records_from_alpha(rays, thres=thres)


def _upstream(rng, R, N):
    gw = np.where(R.flag, rng.standard_normal(R.ray.shape[0]), 0).astype(np.float32)
    return gw, rng.standard_normal(N).astype(np.float32)


def test_float64_chain_equals_autograd():
    """g_alpha and g_d of the oracle against torch float64 autograd of w_i = alpha_i prod_{j<i} (1 - alpha_j + 1e-10) and
    last = prod_j (1 - alpha_j + 1e-10), alpha = 1 - (1 + exp(d + shift))^-interval, on ragged rays: 1e-12 relative.
    alpha is a multiple of 2^-12 so that float32(1 - alpha) is exact; alpha == 1 (1 - alpha == 0: only the 1e-10 is left in
    the denominator) ends some rays."""
    rng = np.random.default_rng(0)
    interval, n_list = 0.5, [1, 2, 63, 64, 65, 130, 7, 300]
    R = _Rec64()
    R.n = np.array(n_list, np.int64)
    R.first = np.concatenate([[0], np.cumsum(R.n)])
    R.ray = np.repeat(np.arange(len(n_list)), R.n)
    R.idx = np.arange(R.ray.shape[0]) - R.first[R.ray]
    alpha = rng.integers(1, 1200, R.ray.shape[0]) / 4096.0
    alpha[R.first[1:][[2, 5]] - 1] = 1.0
    a = torch.tensor(alpha, dtype=torch.float64, requires_grad=True)
    gw, gl = rng.standard_normal(alpha.shape[0]), rng.standard_normal(len(n_list))
    loss, Ts, lasts = 0.0, [], []
    for r, n in enumerate(n_list):
        ar = a[R.first[r]:R.first[r + 1]]
        f = 1.0 - ar + 1e-10
        T = torch.cat([torch.ones(1, dtype=torch.float64), torch.cumprod(f, 0)[:-1]])
        Ts.append(T.detach().numpy()); lasts.append(float(torch.prod(f).detach()))
        loss = loss + (torch.tensor(gw[R.first[r]:R.first[r + 1]]) * T * ar).sum() + gl[r] * torch.prod(f)
    want_ga, = torch.autograd.grad(loss, a)
    R.alpha, R.T = alpha, np.concatenate(Ts)
    R.w = R.T * alpha
    e = np.where(alpha < 1, (1 - np.minimum(alpha, 0.999)) ** (-1 / interval) - 1, 3.0)
    R.exp_d = e
    R.flag = np.ones(alpha.shape[0], bool)
    O = M.density_bwd_reference(R, np.array(lasts), gw, gl, interval)
    np.testing.assert_allclose(O.ga, want_ga.numpy(), rtol=1e-12, atol=0)
    d = torch.tensor(np.log(e), dtype=torch.float64, requires_grad=True)
    al = 1 - (1 + torch.exp(d)) ** (-interval)
    want_gd, = torch.autograd.grad((al * want_ga).sum(), d)
    np.testing.assert_allclose(O.gd, want_gd.numpy(), rtol=1e-12, atol=0)
    assert O.dga.min() > 0 and np.isfinite(O.dga).all() and not O.zero.any()


def _float32_evaluations(R, n3, last, oracle, rng, interval=0.5):
    """-> {name: worst err / bound}; raises when a correct evaluation leaves its bound"""
    N = R.n.shape[0]
    gw, gl = _upstream(rng, R, N)
    out = {}
    for order, name, got in (('tree', 'tree', M.emulate_tree(R, last, gw, gl, interval)),
                             ('serial', 'serial fma', M.serial_c_oracle(oracle, R, last, gw, gl, interval, fma=True)),
                             ('serial', 'serial plain', M.serial_c_oracle(oracle, R, last, gw, gl, interval, fma=False))):
        O = M.density_bwd_reference(R, last, gw, gl, interval, order)
        out[name] = M.check_density_bwd(R, O, got, name)
    # zero rule and grad_last == NULL
    O = M.density_bwd_reference(R, last, np.zeros_like(gw), None, interval)
    assert O.zero.all()
    M.check_density_bwd(R, O, M.emulate_tree(R, last, np.zeros_like(gw), None, interval))
    O = M.density_bwd_reference(R, last, np.zeros_like(gw), gl, interval)
    M.check_density_bwd(R, O, M.emulate_tree(R, last, np.zeros_like(gw), gl, interval), 'gradient on alphainv_last only')
    return out, (gw, gl)


def test_correct_float32_evaluations_stay_inside_on_ragged_rays(oracle):
    """400 rays of 1 to 600 records, alpha up to 0.9, opaque last samples, early stop, with and without the filters: the
    kernel's tree order and the reference's serial order against their own counts, every record compared."""
    rng = np.random.default_rng(1)
    for thres in (0.0, 1e-4):
        R, n3, last = _ragged(rng, 400, 600, thres=thres)
        assert M.check_records(R, np.full(R.n.shape[0], 600), thres, n3, last) == R.ray.shape[0] > 10000
        worst, _ = _float32_evaluations(R, n3, last, oracle, rng)
        O = M.density_bwd_reference(R, last, *_upstream(rng, R, R.n.shape[0]), 0.5)
        print('thres', thres, 'records', R.ray.shape[0], 'worst err/bound', {k: round(v, 3) for k, v in worst.items()},
              'share of records with bound > 1% of |ref|', float((O.dgd > 0.01 * np.abs(O.gd)).mean()))
        assert all(v <= 1 for v in worst.values())


@pytest.mark.parametrize('mutant', ['drop64', 'no_eps', 'T_after'])
def test_wrong_float32_evaluations_fall_outside(mutant):
    rng = np.random.default_rng(2)
    R, n3, last = _ragged(rng, 60, 200, opaque=1.0)
    N = R.n.shape[0]
    gw, gl = _upstream(rng, R, N)
    O = M.density_bwd_reference(R, last, gw, gl, 0.5)
    M.check_density_bwd(R, O, M.emulate_tree(R, last, gw, gl, 0.5))
    with pytest.raises(AssertionError):
        M.check_density_bwd(R, O, M.emulate_tree(R, last, gw, gl, 0.5, mutant=mutant))


def test_exact_checks_reject_wrong_records():
    rng = np.random.default_rng(3)
    R, n3, last = _ragged(rng, 20, 100, thres=1e-4)
    ns = np.full(20, 100)
    M.check_records(R, ns, 1e-4, n3, last)
    i = int(np.nonzero(~R.is_last)[0][5])
    for what in ('T', 'flag', 'step'):
        keep = getattr(R, what).copy()
        getattr(R, what)[i + 1] = {'T': R.T_after[i + 1], 'flag': not R.flag[i + 1], 'step': R.step[i]}[what]
        with pytest.raises(AssertionError):
            M.check_records(R, ns, 1e-4, n3, last)
        setattr(R, what, keep)
    with pytest.raises(AssertionError):
        M.check_records(R, ns, 1e-4, n3, np.nextafter(last, _F(2)))


def test_per_ray_sum_bounds_hold_for_float32_and_reject_a_lost_slice():
    """march_composite's order in numpy float32 (lanes, rounds of four slices, butterfly) stays inside; without slice u == 3
    it does not."""
    rng = np.random.default_rng(4)
    n = np.array([0, 1, 64, 255, 256, 257, 513, 700])
    off3 = np.concatenate([[0], np.cumsum(n)])
    Mn = int(off3[-1])
    w, c = rng.uniform(0, 0.01, Mn).astype(np.float32), rng.uniform(0, 1, (Mn, 3)).astype(np.float32)
    last, bg = rng.uniform(0, 1, n.shape[0]).astype(np.float32), 1.0

    def run(skip=None):
        out = np.zeros((n.shape[0], 3), np.float32)
        for r in range(n.shape[0]):
            acc = np.zeros((64, 3), np.float32)
            for i in range(off3[r], off3[r + 1]):
                u, lane = ((i - off3[r]) // 64) % 4, (i - off3[r]) % 64
                if u != skip:
                    acc[lane] = M.B.fma32(np.full(3, w[i]), c[i], acc[lane])
            for d in (32, 16, 8, 4, 2, 1):
                acc = (acc + acc[np.arange(64) ^ d]).astype(np.float32)
            out[r] = acc[0] + last[r] * _F(bg)
        return out
    print('composite worst err/bound', M.check_composite(w, c, None, off3, last, bg, run()))
    with pytest.raises(AssertionError):
        M.check_composite(w, c, None, off3, last, bg, run(skip=3))


SCENES = C.all_scenes()


@pytest.mark.parametrize('sc', SCENES, ids=[s.name for s in SCENES])
def test_every_row_hits_its_edge_and_float32_stays_inside(sc, oracle):
    q = C.cpu_forward(sc, oracle)
    assert M.check_records(q.R, q.n_steps, sc.thres, q.n3, q.last) == q.R.ray.shape[0]
    for name, target, pred in sc.rows:
        assert pred(q), f'{sc.name}: row {name} ({target}) does not hit its edge on the CPU oracle'
    worst, _ = _float32_evaluations(q.R, q.n3, q.last, oracle, np.random.default_rng(5), sc.interval)
    print(sc.name, 'rows', len(sc.rows), 'records', q.R.ray.shape[0], 'worst err/bound', {k: round(v, 3) for k, v in worst.items()})


def test_nothing_in_the_package_sets_the_timing_experiments():
    """DVGO_TUNE_EXPERIMENT (march_density: results are wrong when non-zero) has no getter; the library starts with 0 and only
    tools/ may set it: no file of the package calls dvgo_set_tuning at all, and the initial table of march.hip holds 0."""
    import glob
    import os
    import re
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'directvoxgo_amd')
    for path in glob.glob(os.path.join(pkg, '**', '*.py'), recursive=True):
        with open(path) as f:
            assert 'dvgo_set_tuning' not in f.read(), path
    with open(os.path.join(pkg, 'csrc', 'march.hip')) as f:
        m = re.search(r'g_tuning\[DVGO_TUNE_COUNT\] = \{([^}]*)\}', f.read())
    assert [int(v) for v in m.group(1).split(',')][4] == 0
