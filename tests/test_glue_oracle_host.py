"""CPU: tests/glue_oracle.py held to independent references, and its checkers shown to reject a wrong kernel, before any
GPU test relies on them.

  * `adam_reference` with `perlr` against the C oracle's `adam_upd` (all three modes, the value set of the GPU tests) and
    against the three steps of the `masked_adam` fixture, bit for bit;
  * the loss oracle's float64 value and gradients against float64 autograd of `train.render_loss`;
  * the restated launch rule of `loss_samples_kernel` with the numbers written out;
  * every checker: it passes the reference (for the loss value a float32 emulation of the kernel's own summation shape)
    and fails the reference corrupted the way one plausible bug would corrupt it;
  * the derived bound of the loss value is useful: bound / |ref| < 1e-4 at every shape the GPU test launches.
"""
import numpy as np
import pytest
import torch

import glue_oracle as G
from conftest import load_golden
from directvoxgo_amd.masked_adam import adam_step_size
from directvoxgo_amd.train import COARSE_TRAIN, FINE_TRAIN, render_loss

_F = np.float32
M_LIST, SHAPES = G.LOSS_M, G.LOSS_SHAPES


def _weights(cfg):
    return cfg['weight_main'], cfg['weight_entropy_last'], cfg['weight_rgbper']


# ------------------------------------------------------------------------------------------ agreement
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_adam_reference_with_perlr_equals_the_c_oracle_on_the_value_set(oracle, mode):
    for n, rot in [(1, 0), (1, 2), (3, 4), (7, 0), (1025, 0), (100003, 0)]:
        for step in (1, 3):
            p, g, m, v, perlr = G.adam_values(n, seed=n + step, rot=rot)
            a = [x.copy() for x in (p, g, m, v)]
            oracle.adam_upd(a[0], a[1], a[2], a[3], step, 0.9, 0.99, 0.1, 1e-8, mode=mode, perlr=perlr if mode == 2 else None)
            exp = G.adam_expected(p, g, m, v, adam_step_size(0.1, 0.9, 0.99, step), mode, perlr)
            G.check_adam((a[0], a[2], a[3]), exp, f'n {n} step {step}')
            assert np.array_equal(G.bits(a[1]), G.bits(g))
    # the value set is what it says it is
    p, g, m, v, perlr = G.adam_values(1024)
    assert G.bits(g[:3]).tolist() == [0, -2 ** 31, 1] and m[3] == 0 and v[3] == 0 and perlr[4] == 0 and g[4] != 0
    grp = g[G.GROUPS_AT:G.N_SPECIAL].reshape(6, 4) != 0
    assert not grp[0].any() and grp[5].all() and np.array_equal(grp[1:5], np.eye(4, dtype=bool))
    p1, m1, v1 = G.adam_expected(p, g, m, v, 0.1, 0)
    assert v1[3] == 0 and m1[3] != 0 and p1[3] != p[3]                   # sqrtf(v) == 0: eps alone divides
    p2, m2, v2 = G.adam_expected(p, g, m, v, 0.1, 2, perlr)
    assert G.bits(p2[4]) == G.bits(p[4]) and m2[4] != m[4] and v2[4] != v[4]     # perlr == 0: p stays, m and v move


def test_adam_reference_reproduces_the_three_fixture_steps_in_every_mode(oracle):
    g = load_golden('masked_adam')
    for tag, mode in (('plain', 0), ('masked', 1), ('perlr', 2)):
        p = g[f'{tag}_p0'].copy()
        m, v = np.zeros_like(p), np.zeros_like(p)
        c = [p.copy(), m.copy(), v.copy()]                            # the same three steps through the C oracle
        perlr = None
        if mode == 2:
            cnt = g['perlr_count'].astype(_F)
            perlr = cnt / cnt.max()
        for s in range(3):
            grad = np.ascontiguousarray(g[f'{tag}_g{s}'], _F)
            p, m, v = G.adam_expected(p, grad, m, v, adam_step_size(0.1, 0.9, 0.99, s + 1), mode, perlr)
            G.assert_bits(p, g[f'{tag}_p{s + 1}'], f'{tag} step {s + 1}')
            oracle.adam_upd(c[0], grad.copy(), c[1], c[2], s + 1, 0.9, 0.99, 0.1, 1e-8, mode=mode, perlr=perlr)
            G.check_adam(c, (p, m, v), f'{tag} step {s + 1}: C oracle')
        G.assert_bits(m, g[f'{tag}_exp_avg'], f'{tag} exp_avg')


@pytest.mark.parametrize('cfg', [FINE_TRAIN, COARSE_TRAIN, dict(FINE_TRAIN, weight_rgbper=0.0), dict(FINE_TRAIN, weight_entropy_last=0.0)])
def test_loss_oracle_equals_float64_autograd_of_render_loss(cfg):
    N, M = 257, 3001
    ins = G.loss_inputs(N, M, seed=3)
    lo, hi = 1e-6, 1 - 1e-6                           # in float64 the closed interval ends on the doubles
    edges64 = np.array([0.0, 1.0, 1e-7, 1 - 1e-7, 0.5, lo, hi, np.nextafter(lo, 0), np.nextafter(lo, 1), np.nextafter(hi, 0),
                        np.nextafter(hi, 1), -0.25, 2.0])
    last64 = ins[1].astype(np.float64)
    last64[:edges64.size] = edges64
    for n_global in (N, 2 * N):
        O = G.loss_oracle(ins[0], last64, *ins[2:], n_global, *_weights(cfg), exact=True)
        t = [torch.from_numpy(np.asarray(x, np.float64)).requires_grad_() for x in (ins[0], last64, ins[3], ins[4])]
        res = {'rgb_marched': t[0], 'alphainv_last': t[1], 'raw_rgb': t[2], 'weights': t[3], 'ray_id': torch.from_numpy(ins[5])}
        loss = render_loss(res, torch.from_numpy(ins[2].astype(np.float64)), n_global, cfg)
        grads = torch.autograd.grad(loss, t, allow_unused=True)
        assert grads[3] is None                                       # weights are detached
        assert abs(float(loss.detach()) - O.ref) <= 1e-12 * abs(O.ref)
        np.testing.assert_allclose(O.grads64[0], grads[0].numpy(), rtol=1e-12, atol=1e-18)
        gl = np.zeros(N) if grads[1] is None else grads[1].numpy()
        np.testing.assert_allclose(O.grads64[1], gl, rtol=1e-12, atol=1e-16)
        if cfg['weight_entropy_last'] > 0:                            # autograd's clamp: closed interval
            assert gl[5] != 0 and gl[6] != 0 and gl[7] == 0 and gl[10] == 0 and gl[8] != 0 and gl[9] != 0
            assert O.inside[[5, 6, 8, 9]].all() and not O.inside[[0, 1, 2, 3, 7, 10, 11, 12]].any()
        if cfg['weight_rgbper'] > 0:
            np.testing.assert_allclose(O.grads64[2], grads[2].numpy(), rtol=1e-12, atol=1e-18)
        else:
            assert O.g_raw is None and (grads[2] is None or float(grads[2].abs().max()) == 0)
        # the kernel-scalar statement differs from the formula by the rounding of 1/n, 1/3, the weights and 1 - p only
        K = G.loss_oracle(*ins, n_global, *_weights(cfg))
        assert abs(K.ref - O.ref) <= 4 * G.U * O.mag
        np.testing.assert_allclose(K.g_marched, O.grads64[0], rtol=8 * G.U, atol=1e-40)
        if K.g_raw is not None:
            np.testing.assert_allclose(K.g_raw, O.grads64[2], rtol=8 * G.U, atol=1e-40)


def test_launch_rule_of_the_sample_kernel_with_the_numbers_written_out():
    assert M_LIST == [1, 255, 256, 257, 65280, 65281, 65536, 65537, 1048575, 1048576, 1048577]
    grids = [G.launch_grid(m) for m in M_LIST]
    assert grids == [1, 1, 1, 2, 255, 256, 256, 256, 256, 1024, 1024]
    for m in M_LIST:                    # the expression of loss.hip:182-183 itself
        nb = (m + 255) // 256
        assert G.launch_grid(m) == (nb if nb < 256 else (1024 if m >= (1 << 20) else 256))
    trips = [-(-m // (g * 256)) for m, g in zip(M_LIST, grids)]
    assert trips == [1, 1, 1, 1, 1, 1, 1, 2, 16, 4, 5]
    assert G.loss_k(257, 65537, 256) == max(9, 8 + 2) + 9 + (2 + 256) + 1
    assert G.loss_k(257, 0, 0, samples=False) == 9 + 9 + 2 + 1 and G.loss_k(0, 5, 1) == 9 + 9 + 1 + 1


# ------------------------------------------------------------------------------------------ the kernel's shape in float32
def _emulate_loss(ins, n_global, w_main, w_ent, w_per, grid, count=None, drop_wg=None, third=True):
    """The two loss kernels in numpy float32 with their own summation shape: per-thread grid-stride accumulation, the
    xor-shuffle tree, the four waves, one addition per workgroup onto the result (rays first, in workgroup order)."""
    rm, last, tgt, raw, w, rid = ins
    N, M = rm.shape[0], raw.shape[0] if count is None else count
    f = _F
    wm, we, wp = f(w_main), f(w_ent), f(w_per)
    inv, th = f(1) / f(n_global), (f(1) / f(3) if third else f(1))

    def se_of(d):
        se = np.zeros(d.shape[0], f)
        for c in range(3):
            se = G.fma32(d[:, c], d[:, c], se)
        return se

    def block_sums(l):                                  # l [n_wg * 256] -> [n_wg]
        v = l.reshape(-1, 4, 64)
        lane = np.arange(64)
        for d in (32, 16, 8, 4, 2, 1):
            v = v + v[:, :, lane ^ d]
        r = v[:, :, 0]
        return ((r[:, 0] + r[:, 1]) + r[:, 2]) + r[:, 3]

    parts = []
    if N:
        l = ((wm * se_of(rm - tgt)) * inv) * th
        if we > 0:
            p = np.minimum(np.maximum(last, G.LO), G.HI)
            q = f(1) - p
            l = l + ((we * (-(p * np.log(p) + q * np.log(q)))) * inv)
        pad = np.zeros(-(-N // 256) * 256, f)
        pad[:N] = l
        parts.append(block_sums(pad))
    if M and wp > 0:
        T = grid * 256
        term = (((wp * w[:M]) * se_of(raw[:M] - tgt[rid[:M]])) * inv)
        trips = -(-M // T)
        pad = np.zeros(trips * T, f)
        pad[:M] = term
        l = np.zeros(T, f)
        for t in range(trips):
            l = l + pad[t * T:(t + 1) * T]
        s = block_sums(l)
        if drop_wg is not None:
            s = np.delete(s, drop_wg)
        parts.append(s)
    out = f(0)
    for s in np.concatenate(parts) if parts else []:
        out = out + s
    return out


@pytest.mark.parametrize('N,M', SHAPES)
def test_loss_bound_holds_for_the_emulated_kernel_and_is_not_vacuous(N, M):
    ins = G.loss_inputs(N, M, seed=N + M)
    for w in (_weights(FINE_TRAIN), _weights(COARSE_TRAIN), (0.7, 0.002, 0.03)):
        for n_global in (N, 2 * N, 3 * N):
            O = G.loss_oracle(*ins, n_global, *w)
            got = _emulate_loss(ins, n_global, *w, O.grid)
            G.check_loss_value(O, got)
            print(f'N {N} M {M} n_global {n_global} weights {w}: k {O.k} bound / |ref| {O.bound / abs(O.ref):.3e}')
            assert O.bound / abs(O.ref) < 1e-4


def test_loss_value_checker_rejects_wrong_sums():
    w = _weights(FINE_TRAIN)
    # one workgroup's partial sum dropped, on the second trip of the grid-stride loop
    N, M = 257, 65537
    ins = G.loss_inputs(N, M, seed=1)
    O = G.loss_oracle(*ins, N, *w)
    G.check_loss_value(O, _emulate_loss(ins, N, *w, O.grid))
    for wg in (0, 255):
        with pytest.raises(AssertionError, match='gamma'):
            G.check_loss_value(O, _emulate_loss(ins, N, *w, O.grid, drop_wg=wg))
    # the missing 1/3
    with pytest.raises(AssertionError, match='gamma'):
        G.check_loss_value(O, _emulate_loss(ins, N, *w, O.grid, third=False))
    # summed over the capacity instead of the count; the rows past the count hold NaN, as in the GPU test
    cap = 70000
    for count in (0, 1, cap - 1):
        ins = G.loss_inputs(N, cap, seed=2)
        ins[3][count:], ins[4][count:] = np.nan, np.nan
        O = G.loss_oracle(*ins, N, *w, count=count)
        assert O.grid == G.launch_grid(cap) and O.M == count and np.isfinite(O.ref)
        G.check_loss_value(O, _emulate_loss(ins, N, *w, O.grid, count=count))
        with pytest.raises(AssertionError, match='value'):
            G.check_loss_value(O, _emulate_loss(ins, N, *w, O.grid, count=cap))
    ins = G.loss_inputs(N, cap, seed=2)                          # ... or finite leftovers of an earlier step
    O = G.loss_oracle(*ins, N, *w, count=cap // 2)
    with pytest.raises(AssertionError, match='gamma'):
        G.check_loss_value(O, _emulate_loss(ins, N, *w, O.grid, count=cap))
    O = G.loss_oracle(*ins, N, *w, count=cap + 5)                 # a count past the capacity clamps to it
    assert O.M == cap
    with pytest.raises(AssertionError, match='value'):
        G.check_loss_value(O, np.nan)


def test_loss_gradient_checkers_reject_wrong_gradients():
    N, M = 65, 300
    ins = G.loss_inputs(N, M, seed=4)
    w = _weights(FINE_TRAIN)
    O = G.loss_oracle(*ins, 2 * N, *w)
    f = _F
    p = np.minimum(np.maximum(ins[1], G.LO), G.HI)
    gl = np.where(O.inside, ((f(w[1]) * (np.log(f(1) - p) - np.log(p))) * O.inv.astype(f)), f(0)).astype(f)
    G.check_loss_grads(O, O.g_marched, gl, O.g_raw)
    # another association of the g_marched product (it needs a 2 w_main that is no power of two to show)
    Oa = G.loss_oracle(*ins, 3 * N, 0.7, w[1], w[2])
    wrong = ((f(2) * f(0.7)) * ((ins[0] - ins[2]) * (f(1) / f(3 * N)))) * (f(1) / f(3))
    assert (G.bits(wrong) != G.bits(Oa.g_marched)).mean() > 0.05
    with pytest.raises(AssertionError, match='g_marched'):
        G.assert_bits(wrong, Oa.g_marched, 'g_marched')
    # the missing 1/3
    d = ins[0] - ins[2]
    with pytest.raises(AssertionError, match='g_marched'):
        G.check_loss_grads(O, ((f(2) * f(w[0])) * d) * (f(1) / f(2 * N)), gl, O.g_raw)
    # another association of the same product is not the kernel's
    with pytest.raises(AssertionError, match='g_raw'):
        G.check_loss_grads(O, O.g_marched, gl, (f(2) * f(w[2])) * (ins[4][:, None] * (ins[3] - ins[2][ins[5]])) * (f(1) / f(2 * N)))
    edge = {float(x): i for i, x in enumerate(G.LAST_EDGES)}
    just_out = [edge[float(np.nextafter(G.LO, f(0)))], edge[float(np.nextafter(G.HI, f(1)))]]
    on = [edge[float(G.LO)], edge[float(G.HI)]]
    assert not O.inside[just_out].any() and O.inside[on].all() and (gl[on] != 0).all()
    for i in just_out:                  # non-zero just outside the clamp (an open/closed mix-up, or a clamp on p not x)
        bad = gl.copy(); bad[i] = gl[on[0]]
        with pytest.raises(AssertionError, match='outside the clamp'):
            G.check_g_last(O, bad)
    for i in on:                        # zero exactly on the clamp constants
        bad = gl.copy(); bad[i] = 0
        with pytest.raises(AssertionError, match='g_last'):
            G.check_g_last(O, bad)
    bad = gl.copy(); bad[0] = f(-0.0)   # a product with a zero instead of the literal 0.0f
    with pytest.raises(AssertionError, match='outside the clamp'):
        G.check_g_last(O, bad)
    with pytest.raises(AssertionError, match='g_last'):          # the sign, and a factor
        G.check_g_last(O, -gl)
    with pytest.raises(AssertionError, match='g_last'):
        G.check_g_last(O, gl * f(1.0001))
    O0 = G.loss_oracle(*ins, 2 * N, w[0], 0.0, w[2])
    G.check_g_last(O0, np.zeros(N, f))
    with pytest.raises(AssertionError, match='outside the clamp'):
        G.check_g_last(O0, gl)


def test_adam_checker_rejects_plausible_kernel_bugs():
    n, ss = 1025, 0.0123
    p, g, m, v, perlr = G.adam_values(n, seed=9)
    exp = G.adam_expected(p, g, m, v, ss, 1)
    G.check_adam(exp, exp, 'reference')
    # the masked skip taken per float4: a group with a non-zero lane has its zero lanes updated too
    plain = G.adam_expected(p, g, m, v, ss, 0)
    grp_any = np.repeat((g[:1024].reshape(-1, 4) != 0).any(1), 4)
    bad = [np.where(np.concatenate([grp_any, [False]]), a, b) for a, b in zip(plain, exp)]
    assert any((G.bits(a) != G.bits(b)).any() for a, b in zip(bad, exp))
    with pytest.raises(AssertionError, match='differ in bits'):
        G.check_adam(bad, exp, 'float4 skip')
    # ... and the other way round: a group with a zero lane skipped as a whole
    grp_all = np.repeat((g[:1024].reshape(-1, 4) != 0).all(1), 4)
    bad = [np.where(np.concatenate([grp_all, [g[1024] != 0]]), b, a) for a, b in zip((p, m, v), exp)]
    with pytest.raises(AssertionError, match='differ in bits'):
        G.check_adam(bad, exp, 'float4 skip')
    # a tail element left untouched (n % 4 == 1)
    exp0 = G.adam_expected(p, g, m, v, ss, 0)
    bad = [a.copy() for a in exp0]
    for a, b in zip(bad, (p, m, v)):
        a[-1] = b[-1]
    with pytest.raises(AssertionError, match='differ in bits'):
        G.check_adam(bad, exp0, 'tail')
    # a perlr that is ignored
    exp2 = G.adam_expected(p, g, m, v, ss, 2, perlr)
    with pytest.raises(AssertionError, match='p'):
        G.check_adam(exp0, exp2, 'perlr')
    # the neighbouring tensor's moment at a tensor boundary (multi-tensor launch)
    a, b = G.adam_values(64, seed=1, scale=1.0), G.adam_values(65, seed=2, scale=100.0)
    eb = G.adam_expected(b[0], b[1], b[2], b[3], ss, 0)
    m_wrong = b[2].copy(); m_wrong[0] = a[2][-1]
    with pytest.raises(AssertionError, match='differ in bits'):
        G.check_adam(G.adam_expected(b[0], b[1], m_wrong, b[3], ss, 0), eb, 'boundary')
    # a written guard
    raw = np.full(20, G.SENTINEL, np.int32)
    raw[4:16] = 0
    G.assert_sentinels(raw, 4, 16, 'guards')
    raw[16] = 0x7fc00000
    with pytest.raises(AssertionError, match='guard'):
        G.assert_sentinels(raw, 4, 16, 'guards')


@pytest.mark.parametrize('F', [1, 4, 10])
def test_viewdir_checker_rejects_every_wrong_layout_in_every_row(F):
    N = 1000
    v, freq = G.viewdir_inputs(N), G.viewdir_freq(F)
    _, fn = G.viewdir_expected(v, freq)
    ok = np.concatenate([v, fn.astype(_F)], 1)
    G.check_viewdir(ok, v, freq)
    assert not G.viewdir_rows_failing(ok, v, freq).any()
    s, c = fn[:, :3 * F], fn[:, 3 * F:]
    wrong = {'swapped': np.concatenate([v, c, s], 1)}
    q = np.arange(3 * F)
    a_fm = (v[:, q % 3] * freq[q // 3]).astype(np.float64)                    # frequency-major
    if F > 1:
        wrong['frequency-major'] = np.concatenate([v, np.sin(a_fm), np.cos(a_fm)], 1)
    for shift in (1, -1):
        qq = (q + shift) % (3 * F)
        wrong[f'q {shift:+d}'] = np.concatenate([v, s[:, qq], c[:, qq]], 1)
    for name, w in wrong.items():
        failing = G.viewdir_rows_failing(w.astype(_F), v, freq)
        assert failing.all(), f'{name}: rows {np.nonzero(~failing)[0][:5].tolist()} would pass'
        with pytest.raises(AssertionError):
            G.check_viewdir(w.astype(_F), v, freq)
    assert G.viewdir_expected(v, None)[1].shape == (N, 0)
    G.check_viewdir(v.copy(), v, None)


def test_padded_layout_checker_rejects_a_touched_pad_channel(oracle):
    C, X, Y, Z = 12, 5, 6, 7
    p, g = G.tv_inputs((1, C, X, Y, Z))
    exp = G.tv_expected(oracle, p, g, 0.3, 0.6, 1.2, True)
    assert (G.bits(exp) != G.bits(g)).any()
    view_of = lambda big: np.moveaxis(big[..., :C], -1, 0)[None]            # noqa: E731  channels-last, 12 of 16
    big = np.full((X, Y, Z, 16), G.SENTINEL, np.int32).view(_F)
    view_of(big)[...] = exp
    G.check_padded(big, view_of, exp, 'tv')
    bad = big.copy(); bad[2, 3, 4, 12] = 0.0                                # a stale pad channel touched
    with pytest.raises(AssertionError, match='padding'):
        G.check_padded(bad, view_of, exp, 'tv')
    bad = big.copy(); bad[2, 3, 4, 11] += _F(1e-3)
    with pytest.raises(AssertionError, match='differ in bits'):
        G.check_padded(bad, view_of, exp, 'tv')
