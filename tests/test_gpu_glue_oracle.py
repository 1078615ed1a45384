"""GPU: the dense Adam kernels, the fused loss, the view embedding, the multi-copy and the flat total-variation kernel held
elementwise to tests/glue_oracle.py (which tests/test_glue_oracle_host.py pins on the CPU), on every dispatch branch.

The kernels are called at the C ABI (`directvoxgo_amd._lib`), so that alignment, guards and the device count are the
test's to choose, and through the Python entry points that training uses.  Everything that does not pass through libm is
compared bit for bit; every buffer a kernel writes lies between guard float4s holding `glue_oracle.SENTINEL`.
"""
import ctypes

import numpy as np
import pytest
import torch

import glue_oracle as G

pytestmark = pytest.mark.gpu

_F = np.float32
SENT = int(G.SENTINEL)
B1, B2, EPS = 0.9, 0.99, 1e-8


@pytest.fixture(scope='module')
def L():
    from directvoxgo_amd import _lib
    _lib.lib()
    return _lib


def rc(L, name, *args):
    """The entry point's own return code (`_lib.call` would raise), after the stream has drained."""
    code = getattr(L.lib(), name)(*args)
    torch.cuda.synchronize()
    return code


def stream(L):
    return L._vp(torch.cuda.current_stream().cuda_stream)


class Buf:
    """A float32 array on the device between two guard float4s of SENTINEL; `offset` floats move its start off the
    16-byte boundary.  Without `arr` the data region itself starts as SENTINEL."""

    def __init__(self, arr=None, n=None, offset=0):
        n = int(np.asarray(arr).size if arr is not None else n)
        self.raw = torch.full((4 + offset + n + 4,), SENT, dtype=torch.int32, device='cuda')
        assert self.raw.data_ptr() % 16 == 0
        self.lo, self.hi, self.n = 4 + offset, 4 + offset + n, n
        self.t = self.raw[self.lo:self.hi].view(torch.float32)
        assert n == 0 or self.t.data_ptr() == self.raw.data_ptr() + 4 * self.lo        # (an empty view has no address)
        if arr is not None and n:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(arr, _F).reshape(-1)))

    def get(self):
        return self.t.cpu().numpy()

    def image(self):
        return self.raw.cpu().numpy()

    def check(self, what):
        G.assert_sentinels(self.image(), self.lo, self.hi, what)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


# ====================================================================================== dvgo_adam_upd
ADAM_N = [1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 4 * 256 + 1, 100003]
# which of (param, grad, exp_avg, exp_avg_sq, perlr) starts one float off the 16-byte boundary (None: the vector branch)
ADAM_CASES = [(mode, mis) for mode in (0, 1, 2) for mis in (None, 0, 1, 2, 3) + ((4,) if mode == 2 else ())]


def _adam_upd(L, bufs, n, ss, mode, sl=slice(None)):
    p, g, m, v, pl = bufs
    return rc(L, 'dvgo_adam_upd', p.t[sl], g.t[sl], m.t[sl], v.t[sl], pl.t[sl] if mode == 2 else None, n, ss, B1, B2, EPS, mode,
              stream(L))


@pytest.mark.parametrize('mode,mis', ADAM_CASES)
def test_adam_upd_every_tail_on_the_vector_and_the_scalar_branch(L, mode, mis):
    """`adam_kernel<mode>`: float4 body and tail loop (all pointers aligned) or one thread per element (any pointer off by
    one float), at every n around the float4 and the workgroup edge; expected bits from `adam_reference`."""
    ss = 0.0123
    for n in ADAM_N:
        for rot in (range(0, G.N_SPECIAL, n) if n < G.N_SPECIAL else (0,)):
            vals = G.adam_values(n, seed=1000 * mode + n, rot=rot)
            bufs = [Buf(a, offset=1 if mis == i else 0) for i, a in enumerate(vals)]
            vec = all(b.t.data_ptr() % 16 == 0 for b in (bufs if mode == 2 else bufs[:4]))
            assert vec == (mis is None)
            assert _adam_upd(L, bufs, n, ss, mode) == 0
            what = f'mode {mode} n {n} rot {rot} misaligned {mis}'
            p, g, m, v, pl = vals
            G.check_adam([bufs[i].get() for i in (0, 2, 3)], G.adam_expected(p, g, m, v, ss, mode, pl), what)
            G.assert_bits(bufs[1].get(), g, what + ': grad')
            G.assert_bits(bufs[4].get(), pl, what + ': perlr')
            for b in bufs:
                b.check(what)


def test_adam_upd_masked_float4_groups_skip_per_element(L):
    """Mode 1, vector branch: a float4 whose gradients are all zero is left alone as a whole; in a float4 with one
    non-zero lane exactly that lane moves, in p, m and v alike."""
    n, ss = 1024, 0.0123
    vals = G.adam_values(n, seed=5)
    bufs = [Buf(a) for a in vals]
    assert _adam_upd(L, bufs, n, ss, 1) == 0
    p, g, m, v, _ = vals
    got = [bufs[i].get() for i in (0, 2, 3)]
    G.check_adam(got, G.adam_expected(p, g, m, v, ss, 1), 'mode 1 groups')
    grp = slice(G.GROUPS_AT, G.N_SPECIAL)
    nz = g[grp] != 0
    assert nz.reshape(6, 4).sum(1).tolist() == [0, 1, 1, 1, 1, 4]
    for name, a, b in zip('pmv', got, (p, m, v)):
        same = G.bits(a[grp]) == G.bits(b[grp])
        assert np.array_equal(same, ~nz), f'{name}: lanes {np.nonzero(same == nz)[0].tolist()} of the float4 groups took the wrong branch'
    zero = g == 0
    assert G.bits(g[:2]).tolist() == [0, -2 ** 31] and zero[:2].all() and not zero[2]        # +0.0, -0.0 skipped; 2^-149 not
    for a, b in zip(got, (p, m, v)):
        assert np.array_equal(G.bits(a[zero]), G.bits(b[zero]))
    assert G.bits(got[1][2]) != G.bits(m[2]) or G.bits(got[2][2]) != G.bits(v[2]) or G.bits(got[0][2]) != G.bits(p[2])


@pytest.mark.parametrize('mode', [1, 2])
def test_adam_upd_shard_by_shard_equals_the_whole_tensor_and_leaves_the_neighbours_alone(L, mode):
    """The `[lo:hi]` form of `MaskedAdam.step_shard`: an odd `lo` takes the scalar branch."""
    n, ss = 4099, 0.0123
    vals = G.adam_values(n, seed=77)
    whole = [Buf(a) for a in vals]
    assert _adam_upd(L, whole, n, ss, mode) == 0
    bufs = [Buf(a) for a in vals]
    before = [vals[i].copy() for i in (0, 2, 3)]
    for lo, hi in ((0, 1001), (1001, 2050), (2050, n)):
        assert (bufs[0].t[lo:hi].data_ptr() % 16 == 0) == (lo % 4 == 0)
        assert _adam_upd(L, bufs, hi - lo, ss, mode, slice(lo, hi)) == 0
        after = [bufs[i].get() for i in (0, 2, 3)]
        exp = G.adam_expected(before[0][lo:hi], vals[1][lo:hi], before[1][lo:hi], before[2][lo:hi], ss, mode, vals[4][lo:hi])
        for name, a, b, e in zip('pmv', after, before, exp):
            G.assert_bits(a[lo:hi], e, f'shard [{lo}:{hi}] {name}')
            G.assert_bits(np.delete(a, np.s_[lo:hi]), np.delete(b, np.s_[lo:hi]), f'outside shard [{lo}:{hi}] {name}')
        before = after
    for i in range(5):
        G.assert_bits(bufs[i].get(), whole[i].get(), f'three shards against one call, buffer {i}')
        bufs[i].check('shards'); whole[i].check('whole')


@pytest.mark.parametrize('mode', [1, 2])
def test_step_shard_on_a_channels_last_grid_parameter(L, mode):
    from directvoxgo_amd.dp import flat_view
    from directvoxgo_amd.masked_adam import MaskedAdam, adam_step_size
    shape = (1, 12, 7, 7, 7)
    n = int(np.prod(shape))
    vals = G.adam_values(n, seed=31)

    def grid(a):             # memory order = the flat value set
        return dev(a).view(1, 7, 7, 7, 12).permute(0, 4, 1, 2, 3)

    p = torch.nn.Parameter(grid(vals[0]))
    assert p.is_contiguous(memory_format=torch.channels_last_3d) and not p.is_contiguous()
    p.grad = grid(vals[1])
    opt = MaskedAdam([{'params': [p], 'lr': 0.1, 'skip_zero_grad': mode == 1}])
    if mode == 2:
        opt.set_pervoxel_lr(grid((np.arange(n) % 17).astype(_F)))
    st = opt._state_of(p)
    flat_view(st['exp_avg']).copy_(dev(vals[2])); flat_view(st['exp_avg_sq']).copy_(dev(vals[3]))
    st['step'] = 1
    fp, fg = flat_view(p.data), flat_view(p.grad)
    before = [vals[0], vals[2], vals[3]]
    ss = adam_step_size(0.1, B1, B2, 2)
    for lo, hi in ((0, 1001), (1001, 2050), (2050, n)):
        st['step'] = 1                                       # every rank takes the same optimizer step
        opt.step_shard(p, fp, fg, lo, hi)
        assert st['step'] == 2
        perlr = flat_view(opt.per_lr).cpu().numpy() if mode == 2 else None
        after = [flat_view(t).cpu().numpy() for t in (p.data, st['exp_avg'], st['exp_avg_sq'])]
        exp = G.adam_expected(before[0][lo:hi], vals[1][lo:hi], before[1][lo:hi], before[2][lo:hi], ss, mode,
                              None if perlr is None else perlr[lo:hi])
        for name, a, b, e in zip('pmv', after, before, exp):
            G.assert_bits(a[lo:hi], e, f'shard [{lo}:{hi}] {name}')
            G.assert_bits(np.delete(a, np.s_[lo:hi]), np.delete(b, np.s_[lo:hi]), f'outside shard [{lo}:{hi}] {name}')
        before = after
    if mode == 2:
        assert float(perlr.min()) == 0.0 and float(perlr.max()) == 1.0


def test_adam_upd_return_codes_without_a_launch(L):
    bufs = [Buf(a) for a in G.adam_values(8)]
    img = [b.image() for b in bufs]
    assert _adam_upd(L, bufs, 0, 0.1, 0) == 0
    assert rc(L, 'dvgo_adam_upd', *[b.t for b in bufs], 8, 0.1, B1, B2, EPS, 3, stream(L)) == G.EINVAL
    assert rc(L, 'dvgo_adam_upd', *[b.t for b in bufs[:4]], None, 8, 0.1, B1, B2, EPS, 2, stream(L)) == G.EINVAL
    assert rc(L, 'dvgo_adam_upd', *[b.t for b in bufs], -1, 0.1, B1, B2, EPS, 0, stream(L)) == G.EINVAL
    for b, i in zip(bufs, img):
        assert np.array_equal(b.image(), i)


# ====================================================================================== dvgo_adam_rows
def _rows_inputs(n_vox, seed, first=0):
    """G [n_vox, 16] with NaN pads and the row patterns from `first` on at rows 0, 1, ...: all zero; feature group k zero
    (k = 0, 1, 2), the others not; every group a single non-zero lane; density zero, features not; the reverse."""
    rng = np.random.default_rng(seed)
    Gr = rng.standard_normal((n_vox, 16)).astype(_F)
    Gr[rng.uniform(size=Gr.shape) < 0.3] = 0
    pats = []
    for j in range(7):
        row = rng.uniform(0.5, 2, 13).astype(_F) * rng.choice([-1, 1], 13).astype(_F)
        if j == 0:
            row[:] = 0
        elif j <= 3:
            row[4 * (j - 1):4 * j] = 0
        elif j == 4:
            keep = row[[1, 6, 8]].copy(); row[:12] = 0; row[[1, 6, 8]] = keep
        elif j == 5:
            row[12] = 0
        else:
            row[:12] = 0
        pats.append(row)
    for j, row in enumerate(pats[first:]):
        if j < n_vox:
            Gr[j, :13] = row
    Gr[:, 13:] = np.nan
    st = [(rng.standard_normal((n_vox, 12)) * s).astype(_F) for s in (1, 0.1)] + [(0.01 * rng.uniform(0.01, 1, (n_vox, 12))).astype(_F)]
    sd = [(rng.standard_normal(n_vox) * s).astype(_F) for s in (1, 0.1)] + [(0.01 * rng.uniform(0.01, 1, n_vox)).astype(_F)]
    for a in st[1:] + sd[1:]:
        a[::5] = 0                                          # first-step moments among the others
    return Gr, st, sd


def _adam_rows(L, Gb, kb, db, n_vox, ss_k, mk, ss_d, md, row_stride=16, C=12):
    return rc(L, 'dvgo_adam_rows', Gb.t, n_vox, row_stride, C, kb[0].t, kb[1].t, kb[2].t, ss_k, mk, db[0].t, db[1].t, db[2].t, ss_d,
              md, B1, B2, EPS, stream(L))


@pytest.mark.parametrize('mk,md', [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_adam_rows_elementwise_with_nan_pad_columns(L, mk, md):
    """`adam_rows_kernel<mk, md>`: twelve feature columns and the density column against `adam_reference` with two
    different step sizes; the pad columns hold NaN and change nothing (same bits as with pads of 0)."""
    ss_k, ss_d = 0.0123, 0.0071
    for n_vox in (1, 15, 16, 17, 63, 64, 65, 1000):
        for first in (range(7) if n_vox == 1 else (0,)):
            Gr, st, sd = _rows_inputs(n_vox, seed=10 * n_vox + first, first=first)
            exp_k, exp_d = G.adam_rows_expected(Gr, *st, ss_k, mk, *sd, ss_d, md)
            runs = []
            for pads in (np.nan, 0.0):
                Gp = Gr.copy(); Gp[:, 13:] = pads
                Gb, kb, db = Buf(Gp), [Buf(a) for a in st], [Buf(a) for a in sd]
                assert _adam_rows(L, Gb, kb, db, n_vox, ss_k, mk, ss_d, md) == 0
                what = f'modes ({mk}, {md}) n_vox {n_vox} pattern {first} pads {pads}'
                G.check_adam([b.get().reshape(n_vox, 12) for b in kb], exp_k, what + ' k0')
                G.check_adam([b.get() for b in db], exp_d, what + ' density')
                G.assert_bits(Gb.get(), Gp.reshape(-1), what + ': G')
                for b in [Gb] + kb + db:
                    b.check(what)
                runs.append([b.get() for b in kb + db])
            for a, b in zip(*runs):
                G.assert_bits(a, b, 'NaN pads against zero pads')


def test_adam_rows_return_codes_write_nothing(L):
    n_vox = 17
    Gr, st, sd = _rows_inputs(n_vox, seed=3)
    Gb, kb, db = Buf(Gr), [Buf(a) for a in st], [Buf(a) for a in sd]
    off = [Buf(st[0], offset=1)] + kb[1:]
    img = [b.image() for b in [Gb] + kb + db + off[:1]]
    assert _adam_rows(L, Gb, kb, db, n_vox, 0.1, 1, 0.1, 1, C=11) == G.ERANGE
    assert _adam_rows(L, Gb, kb, db, n_vox, 0.1, 1, 0.1, 1, row_stride=12) == G.ERANGE
    assert _adam_rows(L, Gb, off, db, n_vox, 0.1, 1, 0.1, 1) == G.EINVAL              # p_k0 off the 16-byte boundary
    assert _adam_rows(L, Gb, kb, db, n_vox, 0.1, 2, 0.1, 1) == G.EINVAL
    assert _adam_rows(L, Gb, kb, db, 0, 0.1, 1, 0.1, 1) == 0
    for b, i in zip([Gb] + kb + db + off[:1], img):
        assert np.array_equal(b.image(), i)


def test_step_grid_rows_three_steps_against_the_reference(L):
    from directvoxgo_amd.dp import flat_view
    from directvoxgo_amd.masked_adam import MaskedAdam, adam_step_size
    X, Y, Z = 5, 6, 7
    n_vox = X * Y * Z
    rng = np.random.default_rng(8)
    k0 = torch.nn.Parameter(dev(rng.standard_normal((1, 12, X, Y, Z)).astype(_F)).contiguous(memory_format=torch.channels_last_3d))
    den = torch.nn.Parameter(dev(rng.standard_normal((1, 1, X, Y, Z)).astype(_F)))
    opt = MaskedAdam([{'params': [den], 'lr': 0.1, 'skip_zero_grad': True}, {'params': [k0], 'lr': 0.07, 'skip_zero_grad': True}])
    assert opt.can_step_grid_rows(den, k0)
    pk, pd = flat_view(k0.data).cpu().numpy().reshape(n_vox, 12), den.data.cpu().numpy().reshape(-1)
    mk, vk, md, vd = np.zeros_like(pk), np.zeros_like(pk), np.zeros_like(pd), np.zeros_like(pd)
    for step in (1, 2, 3):
        Gr, _, _ = _rows_inputs(n_vox, seed=step)
        opt.step_grid_rows(den, k0, dev(Gr))
        (pk, mk, vk), (pd, md, vd) = G.adam_rows_expected(Gr, pk, mk, vk, adam_step_size(0.07, B1, B2, step), 1, pd, md, vd,
                                                          adam_step_size(0.1, B1, B2, step), 1)
        sk, sd = opt.state[k0], opt.state[den]
        G.check_adam([flat_view(t).cpu().numpy().reshape(n_vox, 12) for t in (k0.data, sk['exp_avg'], sk['exp_avg_sq'])],
                     (pk, mk, vk), f'step {step} k0')
        G.check_adam([t.cpu().numpy().reshape(-1) for t in (den.data, sd['exp_avg'], sd['exp_avg_sq'])], (pd, md, vd),
                     f'step {step} density')


# ====================================================================================== dvgo_adam_upd_multi
NUMELS = [1, 63, 64, 65, 255, 256, 257, 1000]
MULTI_LISTS = [[257], [1], [63, 65], [64, 64], [255, 1], [256, 1000],
               [256, 64, 1, 63, 65, 255, 257, 1000, 1, 255, 256, 64, 63, 1000, 65, 257],       # edges: block, wave, inside
               [1] * 16]


def _multi_tensors(numels, seed):
    """Per tensor four guarded buffers p, g, m, v with the tensor's own value scale."""
    out = []
    for k, n in enumerate(numels):
        vals = G.adam_values(n, seed=seed + k, scale=1.3 * 2.0 ** (k - 8), rot=k) if n else [np.zeros(0, _F)] * 5
        out.append((vals, [Buf(a) for a in vals[:4]]))
    return out


def _multi_call(L, tensors, ss_host, ss_dev, n=None, null=()):
    n = len(tensors) if n is None else n
    tab = lambda j: (ctypes.c_void_p * max(n, 1))(*[None if k in null else tensors[k % len(tensors)][1][j].t.data_ptr()   # noqa: E731
                                                     for k in range(n)])
    numel = (ctypes.c_int64 * max(n, 1))(*[tensors[k % len(tensors)][1][0].n for k in range(n)])
    return rc(L, 'dvgo_adam_upd_multi', tab(0), tab(1), tab(2), tab(3), numel, n, ss_host, B1, B2, EPS, ss_dev, stream(L))


@pytest.mark.parametrize('numels', MULTI_LISTS, ids=lambda x: f'{len(x)}x{x[0]}')
@pytest.mark.parametrize('from_device', [False, True])
def test_adam_upd_multi_at_tensor_boundaries_and_the_device_step_size(L, numels, from_device):
    """The linear search for the owning tensor with boundaries inside a wavefront, on a wavefront edge and on a block
    edge; `step_size_dev` is what is read when given (the host value is NaN then), else the host value."""
    ss = 0.0123
    tensors = _multi_tensors(numels, seed=100 * len(numels))
    ss_dev = dev(np.array([ss], _F)) if from_device else None
    assert _multi_call(L, tensors, float('nan') if from_device else ss, ss_dev) == 0
    for k, (vals, bufs) in enumerate(tensors):
        p, g, m, v, _ = vals
        what = f'tensor {k} of {numels}'
        G.check_adam([bufs[i].get() for i in (0, 2, 3)], G.adam_expected(p, g, m, v, ss, 0), what)
        G.assert_bits(bufs[1].get(), g, what + ': grad')
        for b in bufs:
            b.check(what)


def test_adam_upd_multi_return_codes_and_the_empty_tensor(L):
    ss = 0.0123
    tensors = _multi_tensors([64, 5, 65], seed=7)
    img = [b.image() for _, bufs in tensors for b in bufs]
    assert _multi_call(L, tensors, ss, None, n=17) == G.EINVAL
    assert _multi_call(L, tensors, ss, None, n=0) == 0
    assert _multi_call(L, tensors, ss, None, null=(1,)) == G.EINVAL          # NULL with numel > 0
    for b, i in zip([b for _, bufs in tensors for b in bufs], img):
        assert np.array_equal(b.image(), i)
    # numel == 0: the four pointers may be NULL (an empty torch tensor has no memory); the neighbours are updated
    tensors = _multi_tensors([64, 0, 65, 0], seed=9)
    assert torch.empty(0, device='cuda').data_ptr() == 0
    assert _multi_call(L, tensors, ss, None, null=(1, 3)) == 0
    for k in (0, 2):
        (p, g, m, v, _), bufs = tensors[k]
        G.check_adam([bufs[i].get() for i in (0, 2, 3)], G.adam_expected(p, g, m, v, ss, 0), f'tensor {k} beside an empty one')
        for b in bufs:
            b.check(f'tensor {k}')
    assert _multi_call(L, _multi_tensors([0, 0], seed=1), ss, None, null=(0, 1)) == 0


def test_masked_adam_step_batches_twenty_tensors_by_step_count_and_takes_an_empty_one(L):
    """`MaskedAdam.step`: 20 small tensors, one of them a step ahead (its own launch, its own step size), the other 19 in
    chunks of 16 and 3; an empty parameter in the group is accepted.  Per tensor against `adam_reference`, bit for bit."""
    from directvoxgo_amd.masked_adam import MaskedAdam, adam_step_size
    import directvoxgo_amd.masked_adam as MA
    sizes = [NUMELS[k % 8] for k in range(20)]
    vals = [G.adam_values(n, seed=50 + k, scale=1.3 * 2.0 ** (k - 10), rot=k) for k, n in enumerate(sizes)]
    params = [torch.nn.Parameter(dev(v[0])) for v in vals] + [torch.nn.Parameter(torch.empty(0, device='cuda'))]
    opt = MaskedAdam([{'params': params, 'lr': 1e-3, 'skip_zero_grad': False}])
    ahead = 7
    state = [[v[0].copy(), np.zeros_like(v[0]), np.zeros_like(v[0]), 0] for v in vals]
    st = opt._state_of(params[ahead])
    st['exp_avg'].copy_(dev(vals[ahead][2])); st['exp_avg_sq'].copy_(dev(vals[ahead][3])); st['step'] = 1
    state[ahead] = [vals[ahead][0].copy(), vals[ahead][2].copy(), vals[ahead][3].copy(), 1]
    launches = []
    orig = MA.adam_upd_multi
    MA.adam_upd_multi = lambda items, step, *a, **k: (launches.append((len(items), step)), orig(items, step, *a, **k))[1]
    try:
        for it in range(3):
            grads = [G.adam_values(n, seed=500 + 20 * it + k, scale=1.3 * 2.0 ** (k - 10), rot=k)[1] for k, n in enumerate(sizes)]
            for p, g in zip(params, grads):
                p.grad = dev(g)
            params[-1].grad = torch.empty(0, device='cuda')
            del launches[:]
            opt.step()
            assert sorted(launches) == sorted([(16, it + 1), (4, it + 1), (1, it + 2)])       # (19 + the empty one, 1 ahead)
            for k, (p, g) in enumerate(zip(params, grads)):
                s = state[k]
                s[3] += 1
                s[0], s[1], s[2] = G.adam_expected(s[0], g, s[1], s[2], adam_step_size(1e-3, B1, B2, s[3]), 0)
                stt = opt.state[p]
                assert stt['step'] == s[3]
                G.check_adam([t.detach().cpu().numpy() for t in (p, stt['exp_avg'], stt['exp_avg_sq'])], s[:3], f'step {it + 1} tensor {k}')
    finally:
        MA.adam_upd_multi = orig


# ====================================================================================== dvgo_loss_fwd_bwd
M_LIST, SHAPES = G.LOSS_M, G.LOSS_SHAPES
FINE, COARSE = (1.0, 0.001, 0.01), (1.0, 0.01, 0.1)                      # (w_main, w_ent, w_per) of FINE_TRAIN / COARSE_TRAIN
# with w_main = 1 the factor 2 w_main is a power of two and every association of the g_marched product gives the same
# bits: the last set (w_main 0.7, n_rays_global 3 N) is there so that the association of loss.hip:33 is what is compared
WEIGHT_SETS = [(FINE, 1), (COARSE, 2), ((1.0, 0.001, 0.0), 1), ((1.0, 0.0, 0.01), 2), (FINE, 2), (COARSE, 1), ((0.7, 0.002, 0.03), 3)]


def test_weight_sets_are_the_training_configs():
    from directvoxgo_amd.train import COARSE_TRAIN, FINE_TRAIN
    for w, cfg in ((FINE, FINE_TRAIN), (COARSE, COARSE_TRAIN)):
        assert w == (cfg['weight_main'], cfg['weight_entropy_last'], cfg['weight_rgbper'])


class LossRun:
    """One dvgo_loss_fwd_bwd at the C ABI: every output starts as SENTINEL between guards, the loss as NaN."""

    def __init__(self, L, d_ins, N, M, n_global, w, m_dev=None, pass_rays=True):
        rm, last, tgt, raw, wts, rid = d_ins
        self.gm, self.gl, self.gr = Buf(n=3 * N), Buf(n=N), Buf(n=3 * M)
        self.loss = torch.full((1,), float('nan'), device='cuda')
        ray = [rm, last] if pass_rays else [None, None]
        self.rc = rc(L, 'dvgo_loss_fwd_bwd', ray[0], ray[1], tgt, N, raw, wts, rid, M, m_dev, n_global, w[0], w[1], w[2],
                     self.gm.t if N else None, self.gl.t if N else None, self.gr.t if M else None, self.loss, stream(L))

    def check(self, O, what):
        assert self.rc == 0
        ratio = G.check_loss_value(O, self.loss.cpu().numpy()[0], what)
        print(f'{what}: k {O.k} err / bound {ratio:.3f}')
        G.check_loss_grads(O, self.gm.get().reshape(-1, 3), self.gl.get(), self.gr.get().reshape(-1, 3), what)
        rows = O.M if O.g_raw is not None else 0                 # w_per == 0: g_raw is not written at all
        G.assert_sentinels(self.gr.image(), self.gr.lo, self.gr.lo + 3 * rows, what + ': g_raw past the count')
        self.gm.check(what); self.gl.check(what)


def _d(ins):
    return [dev(a) for a in ins]


@pytest.mark.parametrize('N,M', SHAPES)
def test_loss_value_and_gradients_on_every_launch_shape(L, N, M):
    """`nb < 256` launches, the 256-workgroup grid-stride loop (second trip from M = 65537) and the 1024-workgroup launch
    (M >= 2^20); value inside the derived bound, g_marched and g_raw bit for bit, g_last exact zeros / the libm bar."""
    ins = G.loss_inputs(N, M, seed=N + M)
    assert len(np.unique(ins[5])) < N or N < 5
    d_ins = _d(ins)
    for w, mult in WEIGHT_SETS:
        O = G.loss_oracle(*ins, mult * N, *w)
        assert O.grid == (G.launch_grid(M) if w[2] > 0 else 0)
        LossRun(L, d_ins, N, M, mult * N, w).check(O, f'N {N} M {M} n_global {mult * N} weights {w}')


def test_loss_launch_branches_are_the_ones_the_shapes_name():
    assert [G.launch_grid(m) for m in M_LIST] == [1, 1, 1, 2, 255, 256, 256, 256, 256, 1024, 1024]


def test_loss_without_rays_or_without_samples(L):
    N, M = 65, 300
    ins = G.loss_inputs(N, M, seed=2)
    d_ins = _d(ins)
    # N == 0: the sample term alone (the ray pointers may be NULL; `target` still serves the samples)
    O = G.loss_oracle(ins[0][:0], ins[1][:0], ins[2], *ins[3:], N, *FINE)
    assert O.ref > 0 and O.parts[0].size == 0
    LossRun(L, d_ins, 0, M, N, FINE, pass_rays=False).check(O, 'N = 0')
    # M == 0: the ray terms alone
    O = G.loss_oracle(*ins[:3], ins[3][:0], ins[4][:0], ins[5][:0], N, *FINE)
    r = LossRun(L, d_ins[:3] + [None, None, None], N, 0, N, FINE)
    r.check(O, 'M = 0')
    assert rc(L, 'dvgo_loss_fwd_bwd', *d_ins[:3], N, *d_ins[3:], M, None, 0, 1.0, 0.0, 0.0, r.gm.t, r.gl.t, None, r.loss, stream(L)) == G.EINVAL


@pytest.mark.parametrize('cap', [257, 70000])
def test_loss_with_the_sample_count_on_the_device(L, cap):
    """`m_dev`: the rows at and past the count are neither read (they hold NaN) nor written (they keep the sentinel)."""
    N = 257
    for count in (0, 1, cap - 1, cap, cap + 5):
        ins = list(G.loss_inputs(N, cap, seed=cap + count))
        m = min(count, cap)
        ins[3][m:], ins[4][m:] = np.nan, np.nan
        assert ins[5].min() >= 0 and ins[5].max() < N
        m_dev = dev(np.array([count], np.int64))
        for w, mult in ((FINE, 1), (COARSE, 2)):
            O = G.loss_oracle(*ins, mult * N, *w, count=count)
            assert O.M == m and O.grid == G.launch_grid(cap)
            LossRun(L, _d(ins), N, cap, mult * N, w, m_dev=m_dev).check(O, f'cap {cap} count {count} weights {w}')


def test_fused_render_loss_with_n_samples_defines_the_rows_below_the_count(L):
    from directvoxgo_amd.train import FINE_TRAIN, fused_render_loss
    N, cap, count = 257, 70000, 43210
    ins = list(G.loss_inputs(N, cap, seed=11))
    ins[3][count:], ins[4][count:] = np.nan, np.nan
    rm, last, tgt, raw, wts, rid = _d(ins)
    leaves = [rm.requires_grad_(), last.requires_grad_(), raw.requires_grad_()]
    res = {'rgb_marched': rm, 'alphainv_last': last, 'raw_rgb': raw, 'weights': wts, 'ray_id': rid,
           'n_samples': dev(np.array([count], np.int64))}
    loss = fused_render_loss(res, tgt, 2 * N, FINE_TRAIN)
    g = torch.autograd.grad(loss, leaves)
    O = G.loss_oracle(*ins, 2 * N, *FINE, count=count)
    G.check_loss_value(O, float(loss.detach()))
    G.check_loss_grads(O, g[0].cpu().numpy(), g[1].cpu().numpy(), g[2].cpu().numpy()[:count], 'fused_render_loss')


# ====================================================================================== dvgo_viewdir_embed
@pytest.mark.parametrize('F', [0, 1, 4, 10])
def test_viewdir_embed_layout_and_function_values(L, F):
    for N in (1, 255, 256, 257, 1000):
        v = G.viewdir_inputs(N, seed=N)
        freq = G.viewdir_freq(F) if F else None
        E = 3 + 6 * F
        out = Buf(n=N * E)
        assert rc(L, 'dvgo_viewdir_embed', dev(v), dev(freq) if F else None, F, N, out.t, stream(L)) == 0
        G.check_viewdir(out.get().reshape(N, E), v, freq, f'F {F} N {N}')
        out.check(f'F {F} N {N}')
    from directvoxgo_amd.shade import viewdir_embed
    G.check_viewdir(viewdir_embed(dev(v), dev(G.viewdir_freq(F))).cpu().numpy(), v, freq, f'shade.viewdir_embed F {F}')
    assert rc(L, 'dvgo_viewdir_embed', dev(v), None, 2, N, out.t, stream(L)) == G.EINVAL


# ====================================================================================== dvgo_copy_multi
@pytest.mark.parametrize('counts', [[5000], [0], [1, 63, 0, 64], [65, 257, 5000, 1], [257, 0, 0, 64, 63, 1, 5000, 65]],
                         ids=lambda c: f'{len(c)}x{c[0]}')
def test_copy_multi_is_a_bit_exact_copy_between_guards(L, counts):
    rng = np.random.default_rng(len(counts))
    n = len(counts)
    src = [rng.integers(-2 ** 31, 2 ** 31, c, dtype=np.int64).astype(np.int32) for c in counts]          # any bits, NaNs too
    d_src = [dev(s) if s.size else None for s in src]
    dst = [Buf(n=c) for c in counts]
    tab = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() if (t is not None and t.numel()) else None for t in ts])   # noqa: E731
    nd = (ctypes.c_int64 * n)(*counts)
    assert rc(L, 'dvgo_copy_multi', tab([b.t for b in dst]), tab(d_src), nd, n, stream(L)) == 0
    for k, (b, s) in enumerate(zip(dst, src)):
        assert np.array_equal(b.image()[b.lo:b.hi], s), f'tensor {k} of {counts}'
        b.check(f'tensor {k} of {counts}')


def test_copy_multi_rejects_nine_tensors(L):
    dst, src = [Buf(n=4) for _ in range(9)], [dev(np.arange(4, dtype=np.int32)) for _ in range(9)]
    tab = lambda ts: (ctypes.c_void_p * 9)(*[t.data_ptr() for t in ts])          # noqa: E731
    assert rc(L, 'dvgo_copy_multi', tab([b.t for b in dst]), tab(src), (ctypes.c_int64 * 9)(*[4] * 9), 9, stream(L)) == G.EINVAL
    for b in dst:
        G.assert_sentinels(b.image(), b.lo, b.lo, 'nothing copied')


# ====================================================================================== total variation
def _padded(layout, shape, p, g):
    """-> (param view, grad view on the device [1, C, X, Y, Z], the grad allocation, view_of for `check_padded`).  The
    padding of `param` holds NaN, the padding of `grad` SENTINEL."""
    _, C, X, Y, Z = shape
    if layout == 'cf_pad_z':
        big, view_of = (1, C, X, Y, Z + 3), (lambda b: b[..., :Z])
    elif layout == 'cl_pad_c':
        big, view_of = (X, Y, Z, C + 4), (lambda b: (b.permute(3, 0, 1, 2) if torch.is_tensor(b) else np.moveaxis(b, -1, 0))[:C][None])
    else:
        big, view_of = (1, C, X, Y + 2, Z), (lambda b: b[:, :, :, :Y])
    pb = torch.full(big, float('nan'), device='cuda')
    gb = torch.full(big, SENT, dtype=torch.int32, device='cuda').view(torch.float32)
    pv, gv = view_of(pb), view_of(gb)
    pv.copy_(dev(p)); gv.copy_(dev(g))
    assert pv.shape == tuple(shape) and pv.stride() == gv.stride()
    return pv, gv, gb, view_of


TV_PADDED = [('cf_pad_z', (1, 12, 5, 6, 7)), ('cf_pad_z', (1, 3, 4, 3, 70)), ('cf_pad_z', (1, 1, 7, 5, 9)),
             ('cl_pad_c', (1, 12, 5, 6, 7)), ('cl_pad_c', (1, 3, 4, 3, 70)), ('pad_y', (1, 1, 7, 5, 9))]


@pytest.mark.parametrize('layout,shape', TV_PADDED)
@pytest.mark.parametrize('dense', [True, False])
def test_total_variation_flat_kernel_on_layouts_that_are_not_dense_rows(oracle, layout, shape, dense):
    """The fallback `tv_kernel` (both thread orders): channel-first padded in Z, channels-last padded in C, C = 1 padded
    in Y.  The C oracle on a contiguous copy, bit for bit; the padding of `grad` is not written, that of `param` (NaN)
    not read; a slab of such a layout is refused before anything is written."""
    from directvoxgo_amd.ops import total_variation_add_grad
    p, g = G.tv_inputs(shape)
    exp = G.tv_expected(oracle, p, g, 0.3, 0.6, 1.2, dense)
    pv, gv, gb, view_of = _padded(layout, shape, p, g)
    _, C, X, Y, Z = shape
    _, sC, sX, sY, sZ = pv.stride()
    rows_cl = sC == 1 and sZ == C and sY == Z * C and sX == Y * Z * C
    rows_cf = sZ == 1 and sY == Z and sX == Y * Z and (C == 1 or sC == X * Y * Z)
    assert not rows_cl and not rows_cf                       # optim.hip: neither row layout, so the flat kernel runs
    before = gb.cpu().numpy().copy()
    with pytest.raises(RuntimeError, match='32-bit launch range'):
        total_variation_add_grad(pv, gv, 0.3, 0.6, 1.2, dense, x_range=(1, 3))
    torch.cuda.synchronize()
    assert np.array_equal(gb.cpu().numpy().view(np.int32), before.view(np.int32))
    total_variation_add_grad(pv, gv, 0.3, 0.6, 1.2, dense)
    G.check_padded(gb.cpu().numpy(), view_of, exp, f'{layout} {shape} dense {dense}')


TV_WIDTHS = {60: (12, 5), 64: (4, 16), 65: (5, 13), 120: (12, 10), 128: (4, 32), 129: (3, 43), 180: (12, 15), 255: (3, 85),
             256: (4, 64), 257: (257, 1), 600: (12, 50)}          # R = C * K of the channels-last rows


@pytest.mark.parametrize('R', sorted(TV_WIDTHS))
@pytest.mark.parametrize('dense', [True, False])
def test_total_variation_row_kernel_widths(oracle, R, dense):
    """`tv_rows_kernel` in every launch-width class (64 / 128 / 256 threads, and the strided loop above 256) and around
    their edges: channel-first rows of K = R floats and channels-last rows of K * C = R floats."""
    from directvoxgo_amd.ops import total_variation_add_grad
    C, K = TV_WIDTHS[R]
    for fmt, shape in ((torch.contiguous_format, (1, 2, 3, 4, R)), (torch.channels_last_3d, (1, C, 3, 4, K))):
        p, g = G.tv_inputs(shape, seed=R)
        exp = G.tv_expected(oracle, p, g, 0.3, 0.6, 1.2, dense)
        pt, gt = dev(p).contiguous(memory_format=fmt), dev(g).contiguous(memory_format=fmt)
        total_variation_add_grad(pt, gt, 0.3, 0.6, 1.2, dense)
        G.assert_bits(gt.cpu().numpy(), exp, f'R {R} {fmt} dense {dense}')
