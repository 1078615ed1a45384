"""Elementwise statement of the small streaming kernels of a training step (test infrastructure, CPU only, numpy).

It covers `dvgo_adam_upd` / `dvgo_adam_rows` (csrc/optim.hip), `dvgo_adam_upd_multi`, `dvgo_loss_fwd_bwd`,
`dvgo_viewdir_embed`, `dvgo_copy_multi` (csrc/loss.hip) and the flat fallback of `dvgo_total_variation_add_grad_slab`.
`fma32`, `gamma`, U, SLACK, TINY and `adam_reference` are tests/brick_oracle.py's; nothing of them is restated here.

Arithmetic relied on (all the project's own): the library is built with -ffp-contract=off (build.py), so a fused
multiply-add exists only where the source writes `fmaf`; float32 + - * / and sqrtf are correctly rounded and subnormals
are kept.  Whatever does not pass through logf / sinf / cosf is therefore compared BIT FOR BIT (as int32 patterns, so
that -0.0, NaN payloads and subnormals count) with a float32 numpy restatement, operation for operation.  Values that
pass through libm get BASELINE.md section 2's bar for such values, rtol 1e-5 / atol 1e-6 on the function value
(LIBM_R, LIBM_A), carried through the float32 operations that follow.  No constant here was fitted to GPU output.

a. Adam, three entry points, one rule.  `adam_kernel<0|1|2>` and `adam_rows_kernel` call `adam_one` (common.h);
   `adam_multi_kernel` writes the same operations in the same order (loss.hip:118-123: fmaf, fmaf, product, sqrtf, sum,
   quotient, difference).  Expected p, m, v = `brick_oracle.adam_reference` (mode 2: ss = fl(step_size * perlr)), equal
   to the device's as bit patterns.  The float4 early-out of the vector branch (all four gradients == 0) and the
   per-group early-out of the rows kernel skip exactly the elements the per-element rule of `adam_one<1>` skips, so the
   reference knows one masked rule: an element is skipped iff its gradient == 0.0f (+0.0 and -0.0; a subnormal is not
   zero).  Elements a call does not own (guards, the other shards, pad columns) keep their bits.
   SENTINEL = 0x7fa5a5a5 is a NaN with a payload.  The inputs are finite, sqrtf sees v >= 0 and eps > 0 keeps every
   divisor away from 0, so no update produces a NaN at all, and an arithmetic NaN would be the canonical quiet
   0x7fc00000: a sentinel can only be lost by being overwritten.

b. Loss gradients without libm (loss.hip:31-33, 70-72), float32, left to right as the source associates them:
       g_marched[r, c] = fl(fl(fl(fl(2 w_main) d) inv) third),  d = fl(rgb_marched - target)
       g_raw[i, c]     = fl(fl(fl(fl(2 w_per) w_i) d) inv),      d = fl(raw_rgb - target[ray_id_i])
   inv = fl(1 / fl(n_rays_global)), third = fl(1.0f / 3.0f), the weights as float32.  Bit for bit.

c. g_last (loss.hip:36-45).  Exactly 0.0 for every ray when w_ent is not > 0, and where x < 1e-6f or x > fl(1 - 1e-6f)
   (LO, HI as float32; x bit-equal to either is inside: clamp passes the gradient on the closed interval).  Inside,
   p = x, q = fl(1 - p), and with lp, lq the float64 logs of those two float32 numbers
       |got - w_ent (lq - lp) inv| <= w_ent inv ((LIBM_R + gamma(3)) (|lp| + |lq|) + 2 LIBM_A):
   the two logf are at the libm bar, three float32 operations follow (difference, two products); the bound is relative
   to |lp| + |lq| because lq - lp cancels at p = 0.5.  An inside ray's gradient must also be non-zero unless the bound
   itself admits 0 (only around p = 0.5).

d. Loss value.  Terms, in float64 from the float32 inputs with the kernel's float32 scalars:
       ray r      w_main (sum_c d_c^2) inv third  +  w_ent (-(p lp + q lq)) inv      d in float64, q = fl(1 - p)
       sample i   w_per w_i (sum_c d_c^2) inv
   ref = their sum, mag = the sum of the absolute values of the three kinds of term.  (q is the float32 number the
   kernel takes the logarithm of: the rounding of 1 - p is an input of logf, as in c.  `exact=True` evaluates the
   mathematical formula instead -- float64 inputs, 1/n, 1/3, q = 1 - p and the clamp constants as doubles -- and is what
   the host test compares with float64 autograd of train.render_loss.)
   Roundings on a term's own expression, counted from the source:
       main     d (enters squared: 2), three fmaf (3), three products (3)                     8
       entropy  p lp, q lq, their sum (same sign, nothing cancels), w_ent *, * inv            5, then `l +=`: 1
                -> a ray's l carries at most K_RAY = 9 (the main term passes `l +=` too)
       sample   d (2), three fmaf (3), w_per w, * se, * inv (3)                                K_SAMPLE = 8
   Libm: each logf is within LIBM_R |log| + LIBM_A = LIBM_R (|log| + 0.1), so the entropy share moves by at most
   LIBM_R mag_ent, mag_ent = w_ent inv sum_r (p (|lp| + 0.1) + q (|lq| + 0.1)).
   Additions on the path of a term to the result: at most trips = ceil(M / (grid 256)) in the grid-stride loop (rays:
   none), 6 shuffle additions, 3 across the four waves, and one atomic per workgroup of both kernels in any order,
   A = ceil(N / 256) [N > 0] + grid [samples launched]; every partial sum is bounded by mag, so (Higham, Lemma 3.1)
       |got - ref| <= gamma(k) mag + LIBM_R mag_ent + k TINY,    k = max(K_RAY, K_SAMPLE + trips) + 9 + A + SLACK.
   `launch_grid` restates the host's choice of grid (loss.hip:182-183).  With a device count (`m_dev`) the grid comes from
   the capacity, the trips from min(count, capacity) -- the rows at and past the count are neither read nor written.

e. View embedding (loss.hip:85-97).  Columns 0..2 bit-equal to the input; column 3 + q the sine and column 3 + 3F + q the
   cosine of a = fl(v[q / F] * freq[q % F]) (component-major; the float32 product restated exactly), each within
   LIBM_R |f| + LIBM_A of the float64 function of that float32 a.

f. `dvgo_copy_multi`: a bit-exact copy.  Flat `tv_kernel`: the C oracle's `total_variation_add_grad` on a contiguous
   copy, bit for bit (same operations in the same order per element as the row kernels test_total_variation pins).
"""
import numpy as np

from brick_oracle import SLACK, TINY, U, adam_reference, fma32, gamma  # noqa: F401  (U, fma32: for the tests)

_F = np.float32
LIBM_R, LIBM_A = 1e-5, 1e-6
SENTINEL = np.int32(0x7fa5a5a5)
LO, HI = _F(1e-6), _F(1.0) - _F(1e-6)
K_RAY, K_SAMPLE = 9, 8
EINVAL, ERANGE = -1, -2


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def assert_bits(got, exp, what):
    """got == exp as int32 patterns, elementwise; the message names the first offenders."""
    got, exp = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(exp, np.float32)
    assert got.shape == exp.shape, f'{what}: shape {got.shape} != {exp.shape}'
    bad = bits(got) != bits(exp)
    if bad.any():
        idx = np.argwhere(bad)[:5]
        rows = [(tuple(int(i) for i in ix), float(got[tuple(ix)]), float(exp[tuple(ix)])) for ix in idx]
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.size} elements differ in bits; first (index, got, expected): {rows}')


def assert_sentinels(raw, lo, hi, what):
    """raw: int32 image of a whole guarded buffer; everything outside [lo, hi) still holds SENTINEL."""
    raw = np.asarray(raw).view(np.int32).reshape(-1)
    out = np.ones(raw.shape, bool)
    out[lo:hi] = False
    bad = out & (raw != SENTINEL)
    assert not bad.any(), f'{what}: guard elements {np.nonzero(bad)[0][:8].tolist()} were written'


# ------------------------------------------------------------------------------------------ a. Adam
HYPER = dict(b1=0.9, b2=0.99, eps=1e-8)
SUBNORMAL = np.array([1], np.int32).view(np.float32)[0]          # 2^-149
# float4 groups of gradients for the masked vector branch, from element 8 on: all zero; zero except lane k; all non-zero
GROUPS_AT = 8
N_SPECIAL = GROUPS_AT + 4 * 6


def adam_values(n, seed=0, scale=1.0, rot=0):
    """p, g, m, v, perlr [n] float32 with the value set of every Adam test at known positions (entry (j + rot) % 32 of
    the list below lands on element j % n, so a short input meets the later entries through `rot`):
        0  g = +0.0        1  g = -0.0        2  g = 2^-149 (not zero: updated in mode 1)
        3  p = m = v = 0, g = 1e-24: v stays 0 (the square underflows), sqrtf(v) = 0 and eps alone divides
        4  perlr = 0, g != 0   5  perlr = 0, g = 0   6  m = v = 0, g = 2^-149   7  m = v = 0 (a first step)
        8..31  six float4 groups: all zero, zero except lane k (k = 0..3), all non-zero
    Elsewhere g ~ scale N(0, 1) with a quarter exactly 0, m ~ 0.1 scale N, v ~ 0.01 scale^2 U (non-zero moments: second
    and third steps), every seventh element m = v = 0, perlr ~ U[0, 1]."""
    rng = np.random.default_rng(seed)
    s = _F(scale)
    p = (rng.standard_normal(n) * s).astype(_F)
    g = (rng.standard_normal(n) * s).astype(_F)
    g[rng.uniform(size=n) < 0.25] = 0
    m = (0.1 * rng.standard_normal(n) * s).astype(_F)
    v = (0.01 * rng.uniform(0.01, 1, n) * s * s).astype(_F)
    m[6::7] = 0; v[6::7] = 0
    perlr = rng.uniform(0, 1, n).astype(_F)
    nz = lambda: _F(s * rng.uniform(0.5, 2) * rng.choice([-1, 1]))          # noqa: E731
    special = [dict(g=_F(0.0)), dict(g=_F(-0.0)), dict(g=SUBNORMAL), dict(g=_F(1e-24), m=0, v=0, p=0), dict(g=nz(), perlr=0),
               dict(g=_F(0.0), perlr=0), dict(g=SUBNORMAL, m=0, v=0), dict(g=nz(), m=0, v=0)]
    for grp in range(6):
        for lane in range(4):
            zero = grp == 0 or (1 <= grp <= 4 and lane != grp - 1)
            special.append(dict(g=_F(0.0) if zero else nz()))
    assert len(special) == N_SPECIAL
    arrays = dict(p=p, g=g, m=m, v=v, perlr=perlr)
    for j in reversed(range(N_SPECIAL)):                    # reversed: on a short input the earlier positions win
        e, sp = j % n, special[(j + rot) % N_SPECIAL]
        for k, val in sp.items():
            arrays[k][e] = val
    return p, g, m, v, perlr


def adam_expected(p, g, m, v, ss, mode, perlr=None, b1=0.9, b2=0.99, eps=1e-8):
    """-> (p1, m1, v1): fresh arrays, the inputs untouched."""
    p1, m1, v1 = (np.array(x, np.float32, copy=True) for x in (p, m, v))
    adam_reference(p1, np.asarray(g, np.float32), m1, v1, ss, b1, b2, eps, mode == 1, perlr if mode == 2 else None)
    return p1, m1, v1


def check_adam(got, exp, what):
    for name, a, b in zip('pmv', got, exp):
        assert_bits(a, b, f'{what}: {name}')


def adam_rows_expected(G, pk, mk, vk, ss_k, mode_k, pd, md, vd, ss_d, mode_d, b1=0.9, b2=0.99, eps=1e-8):
    """G [n_vox, 16]; pk, mk, vk [n_vox, 12]; pd, md, vd [n_vox].  Columns 13..15 of G are never read.
    -> ((pk1, mk1, vk1), (pd1, md1, vd1))"""
    G = np.asarray(G, np.float32)
    k = adam_expected(pk, G[:, :12], mk, vk, ss_k, mode_k, None, b1, b2, eps)
    d = adam_expected(pd, G[:, 12], md, vd, ss_d, mode_d, None, b1, b2, eps)
    return k, d


# ------------------------------------------------------------------------------------------ b-d. loss
def launch_grid(M):
    """Workgroups of loss_samples_kernel for M rows: loss.hip:182-183,
    `nb = dvgo_blocks(M, 256); grid = nb < 256 ? nb : (M >= (1 << 20) ? 1024 : 256)`."""
    nb = (M + 255) // 256
    return nb if nb < 256 else (1024 if M >= (1 << 20) else 256)


def loss_k(N, M, grid, samples=True):
    """The rounding count of d.: (N rays, M rows actually summed, grid of the samples launch)."""
    samples = samples and M > 0
    trips = -(-M // (grid * 256)) if samples else 0
    A = (-(-N // 256) if N > 0 else 0) + (grid if samples else 0)
    return max(K_RAY, K_SAMPLE + trips if samples else 0) + 9 + A + SLACK


class Loss:
    """What `loss_oracle` returns.  g_marched, g_raw: float32 (bit-exact expectation); g_last_ref, g_last_bound, inside:
    float64 / bool per ray; ref, mag, mag_ent, k, bound of the value; grads64: float64 gradients (host comparison)."""


def loss_oracle(rgb_marched, last, target, raw, weights, ray_id, n_global, w_main, w_ent, w_per, count=None, cap=None,
                exact=False):
    """Inputs as the kernel takes them (float32 arrays, int64 ray_id).  `count`: only the first `count` rows of the
    sample arrays exist for the loss (the device count, already clamped to the capacity `cap`, which sets the grid)."""
    f8 = np.float64
    ft = f8 if exact else _F                 # `exact`: the inputs are float64 numbers and the clamp constants doubles
    lo, hi = (1e-6, 1 - 1e-6) if exact else (LO, HI)
    rm, last, target = (np.asarray(x, ft) for x in (rgb_marched, last, target))
    raw, weights, ray_id = np.asarray(raw, ft), np.asarray(weights, ft), np.asarray(ray_id, np.int64)
    N, M_cap = rm.shape[0], raw.shape[0] if cap is None else cap
    tr = target[:N]                          # (N == 0: `target` still serves the samples)
    M = M_cap if count is None else min(int(count), M_cap)
    raw, weights, ray_id = raw[:M], weights[:M], ray_id[:M]
    wm, we, wp = _F(w_main), _F(w_ent), _F(w_per)
    inv32, third32 = _F(1.0) / _F(n_global), _F(1.0) / _F(3.0)
    if exact:
        inv, third, wm8, we8, wp8 = 1.0 / n_global, 1.0 / 3.0, float(w_main), float(w_ent), float(w_per)
    else:
        inv, third, wm8, we8, wp8 = f8(inv32), f8(third32), f8(wm), f8(we), f8(wp)
    O = Loss()
    O.N, O.M, O.inv, O.w_ent = N, M, f8(inv32), f8(we)
    ent_on, per_on = bool(we > 0), bool(wp > 0) and M_cap > 0
    # ---- gradients, float32, bit for bit
    d32 = rm - tr
    O.g_marched = (((_F(2.0) * wm) * d32) * inv32) * third32
    ds32 = raw - target[ray_id] if M else np.zeros((0, 3), _F)
    O.g_raw = ((((_F(2.0) * wp) * weights)[:, None] * ds32) * inv32) if per_on else None
    # ---- g_last
    x = last
    p = np.minimum(np.maximum(x, lo), hi)
    q = _F(1.0) - p
    O.inside = ((x >= lo) & (x <= hi)) if ent_on else np.zeros(N, bool)
    q8 = (1.0 - p.astype(f8)) if exact else q.astype(f8)
    lp, lq = np.log(p.astype(f8)), np.log(q8)
    O.g_last_ref = np.where(O.inside, we8 * (lq - lp) * inv, 0.0)
    O.g_last_bound = np.where(O.inside, we8 * inv * ((LIBM_R + gamma(3)) * (np.abs(lp) + np.abs(lq)) + 2 * LIBM_A), 0.0)
    # ---- value
    d8 = rm.astype(f8) - tr.astype(f8)
    main = wm8 * (d8 * d8).sum(1) * inv * third
    ent = we8 * -(p.astype(f8) * lp + q8 * lq) * inv if ent_on else np.zeros(N)
    ds8 = raw.astype(f8) - target.astype(f8)[ray_id] if M else np.zeros((0, 3))
    per = wp8 * weights.astype(f8) * (ds8 * ds8).sum(1) * inv if per_on else np.zeros(0)
    O.ref = float(main.sum() + ent.sum() + per.sum())
    O.mag = float(np.abs(main).sum() + np.abs(ent).sum() + np.abs(per).sum())
    O.mag_ent = float((we8 * inv * (p.astype(f8) * (np.abs(lp) + 0.1) + q8 * (np.abs(lq) + 0.1))).sum()) if ent_on else 0.0
    O.grid = launch_grid(M_cap) if per_on else 0
    O.k = loss_k(N, M, O.grid, per_on)
    O.bound = float(gamma(O.k) * O.mag + LIBM_R * O.mag_ent + O.k * TINY)
    O.parts = (main, ent, per)
    # float64 gradients (what autograd of the formula gives)
    O.grads64 = (2.0 * wm8 * d8 * inv * third, O.g_last_ref,
                 (2.0 * wp8 * weights.astype(f8)[:, None] * ds8 * inv) if per_on else None)
    return O


def check_loss_value(O, got, what='loss'):
    got = float(got)
    assert np.isfinite(got), f'{what}: value {got}'
    err = abs(got - O.ref)
    assert err <= O.bound, f'{what}: |{got!r} - {O.ref!r}| = {err:.3e} > gamma({O.k}) mag + 1e-5 mag_ent = {O.bound:.3e}'
    return err / O.bound if O.bound > 0 else 0.0


def check_g_last(O, got, what='g_last'):
    got32 = np.asarray(got, _F)
    got = got32.astype(np.float64)
    out = ~O.inside
    bad = out & (bits(got32) != 0)
    assert not bad.any(), f'{what}: rays {np.nonzero(bad)[0][:5].tolist()} outside the clamp (or w_ent == 0) are not exactly +0.0'
    err = np.abs(got - O.g_last_ref)
    bad = O.inside & ~(err <= O.g_last_bound)
    assert not bad.any(), (f'{what}: rays {np.nonzero(bad)[0][:5].tolist()}: got {got[bad][:5]}, expected '
                           f'{O.g_last_ref[bad][:5]} within {O.g_last_bound[bad][:5]}')
    must = O.inside & (np.abs(O.g_last_ref) > O.g_last_bound)
    bad = must & (got == 0)
    assert not bad.any(), f'{what}: rays {np.nonzero(bad)[0][:5].tolist()} inside the clamp have a zero gradient'


def check_loss_grads(O, g_marched, g_last, g_raw, what='loss'):
    """g_raw: the rows below the count only (the caller checks the sentinels of the rest)."""
    assert_bits(g_marched, O.g_marched, f'{what}: g_marched')
    check_g_last(O, g_last, f'{what}: g_last')
    if O.g_raw is not None:
        assert_bits(np.asarray(g_raw)[:O.M], O.g_raw, f'{what}: g_raw')


# the shapes of the loss tests: N around the workgroup edge at M = 3001; M around every launch branch at N = 257
# (65280: the last `nb < 256` launch, 65537: the first second trip of the grid-stride loop, 2^20: the first 1024-block launch)
LOSS_N = [1, 63, 64, 65, 255, 256, 257, 777]
LOSS_M = [1, 255, 256, 257, 65280, 65281, 65536, 65537, 2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1]
LOSS_SHAPES = [(n, 3001) for n in LOSS_N] + [(257, m) for m in LOSS_M]

LAST_EDGES = np.array([0.0, 1.0, 1e-7, 1 - 1e-7, 0.5, LO, HI, np.nextafter(LO, _F(0)), np.nextafter(LO, _F(1)),
                       np.nextafter(HI, _F(0)), np.nextafter(HI, _F(1)), -0.25, 2.0], _F)


def loss_inputs(N, M, seed=0):
    """rgb_marched, last, target [N..], raw, weights, ray_id [M..]: `last` starts with LAST_EDGES (as many as fit),
    ray_id is sorted, every fifth ray has no sample and (for M >= 4096) ray N // 2 holds a third of all samples."""
    rng = np.random.default_rng(seed)
    rm, tgt = rng.uniform(0, 1, (N, 3)).astype(_F), rng.uniform(0, 1, (N, 3)).astype(_F)
    last = rng.uniform(0, 1, N).astype(_F)
    k = min(N, LAST_EDGES.size)
    last[:k] = LAST_EDGES[:k]
    raw = rng.uniform(0, 1, (M, 3)).astype(_F)
    w = (rng.uniform(0, 1, M) * 0.05).astype(_F)
    if N:
        rays = np.array([r for r in range(N) if r % 5 != 4 or N < 5], np.int64)
        rid = rng.choice(rays, M)
        if M >= 4096:
            rid[:M // 3] = rays[len(rays) // 2]
        rid = np.sort(rid)
    else:
        rid = np.zeros(M, np.int64)
    return rm, last, tgt, raw, w, rid


# ------------------------------------------------------------------------------------------ e. view embedding
def viewdir_inputs(N, seed=0):
    """Unit directions; the first rows are the six axis directions (exact 0 and +-1 components)."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((N, 3))
    v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(_F)
    axes = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]], _F)
    v[:min(N, 6)] = axes[:N]
    return v


def viewdir_freq(F):
    return np.array([2.0 ** i for i in range(F)], _F)          # the model's own (dvgo.py: 2^i, i < viewbase_pe)


def viewdir_expected(v, freq):
    """-> (exact [N, 3] float32, fn [N, 6F] float64: sines then cosines of the float32 angles)"""
    v = np.asarray(v, _F)
    F = 0 if freq is None else len(freq)
    if F == 0:
        return v, np.zeros((v.shape[0], 0))
    a = (v[:, :, None] * np.asarray(freq, _F)[None, None, :]).reshape(v.shape[0], 3 * F).astype(np.float64)
    return v, np.concatenate([np.sin(a), np.cos(a)], 1)


def check_viewdir(got, v, freq, what='viewdir_embed'):
    got = np.asarray(got, _F)
    exact, fn = viewdir_expected(v, freq)
    assert got.shape == (exact.shape[0], 3 + fn.shape[1]), f'{what}: shape {got.shape}'
    assert_bits(got[:, :3], exact, f'{what}: columns 0..2')
    err = np.abs(got[:, 3:].astype(np.float64) - fn)
    bad = ~(err <= LIBM_R * np.abs(fn) + LIBM_A)
    if bad.any():
        ix = np.argwhere(bad)[:5]
        raise AssertionError(f'{what}: {int(bad.sum())} values outside rtol 1e-5 / atol 1e-6; first (row, column - 3): {ix.tolist()}')


def viewdir_rows_failing(got, v, freq):
    """bool [N]: rows of `got` with at least one value outside the bar (host test: every row of a wrong layout)."""
    exact, fn = viewdir_expected(v, freq)
    got = np.asarray(got, _F)
    bad = ~(np.abs(got[:, 3:].astype(np.float64) - fn) <= LIBM_R * np.abs(fn) + LIBM_A)
    return bad.any(1) | (bits(got[:, :3]) != bits(exact)).any(1)


# ------------------------------------------------------------------------------------------ f. total variation
def tv_expected(oracle, p, grad, wx, wy, wz, dense):
    """p, grad: numpy [1, C, X, Y, Z] (any strides) -> the C oracle's result on contiguous copies."""
    exp = np.ascontiguousarray(grad, np.float32).copy()
    oracle.total_variation_add_grad(np.ascontiguousarray(p, np.float32), exp, wx, wy, wz, dense)
    return exp


def tv_inputs(shape, seed=80):
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal(shape) * 2).astype(_F)
    g = rng.standard_normal(shape).astype(_F)
    g[rng.random(shape) < 0.6] = 0
    return p, g


def check_padded(big_after, view_of, exp, what):
    """A strided view of a larger allocation: `view_of(big)` -> the [1, C, X, Y, Z] view.  The view equals `exp` bit for
    bit and every other element of the allocation still holds SENTINEL."""
    big_after = np.asarray(big_after, np.float32)
    assert_bits(np.ascontiguousarray(view_of(big_after)), exp, what)
    rest = bits(big_after).copy().reshape(big_after.shape)
    view_of(rest)[...] = SENTINEL
    bad = rest != SENTINEL
    assert not bad.any(), f'{what}: {int(bad.sum())} padding elements were written, first {np.argwhere(bad)[:4].tolist()}'
