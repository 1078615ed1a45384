"""The positional-encoding colour head kernels (csrc/shade_pe.hip) against the float64 oracle of tests/posenc_oracle.py.

rgb, H1, H2, gz and G1 are held per row to K_ROW * 2^-24 * magnitude, the six weight / bias gradients to K_SUM * 2^-24 *
magnitude, and the ReLU sign bits must equal the oracle's decisions exactly (posenc_oracle.py and shade_oracle.py justify
both K).  Each batch is drawn tie-free first: of 2M + 64 candidate rows those whose ReLU margin is within the bound are
dropped and the first M survivors kept.  The cases call the C ABI the way directvoxgo_amd/shade.py does, but with arrays
the test owns: every output has 64 extra rows filled with a sentinel, the partial records and the total start as NaN.

Branch -> case that reaches it:
  pe_wgrad_kernel n_x_tiles = 1 / 2 / 3                      test_input_widths[P1-E3-dIn12], [P4-E5-dIn32] / [P4-E6-dIn33] ..
                                                             [P9-E7-dIn64] / [P9-E8-dIn65] .. [P15-E3-dIn96]
  exact x-tile boundaries d_in = 32 | 33 and 64 | 65         test_input_widths[P4-E5-dIn32] | [P4-E6-dIn33], [P9-E7-dIn64] | [P9-E8-dIn65]
  odd d_in: zero-padded half k-step S1 = (d_in + 1) / 2,     test_input_widths[P4-E6-dIn33], [P9-E8-dIn65], [P15-E2-dIn95];
    feature kind 4                                           test_partition_edges[P15-E2-*]
  d_in = 96, the maximum (no padding column anywhere)        test_input_widths[P15-E3-dIn96]
  P = 15: arguments up to 2^14 * 1.5 rad                     test_input_widths[P15-*], test_partition_edges[P15-E2-*]
  32-row tiles: a tail of 1, 2, 31, a full tile, 32 + 1      test_partition_edges[*-1], [*-2], [*-31], [*-32], [*-33]
  256-row workgroups (8 waves) of forward / backward         test_partition_edges[*-255], [*-256], [*-257]
  pe_reduce_kernel: n_parts = 16 (slices of one part),       test_partition_edges[*-512],
    17 (slices of two, one of one, seven empty),             [*-513],
    49 (per = 4: the first 4-way unrolled slice)             [*-1567]
  n_parts clamped at 512 / a workgroup with two tiles        test_partition_edges[*-16384] / [*-16385]
  grid-stride loop of forward / backward: exactly one pass   test_partition_edges[*-65536] /
    of 256 workgroups / the second pass                      [*-65537]
  n_parts from the caller: 1 (fifteen empty slices), 3, 7,   test_n_parts_chosen_by_the_caller[40], [1000], [1025]
    16, 17, 50, 512; workgroups that own no tile (M = 40 has
    two tiles), slices of 1, 2, 3 parts beside the 4-way loop
  forward with H1 == nullptr (every render)                  test_forward_without_activations_gives_the_same_bits
  M == 0 at the ABI and through autograd                     test_empty_batch_at_the_abi, test_empty_batch_through_autograd
  argument checks that return before a launch                test_return_codes_without_a_launch
"""
import numpy as np
import pytest
import torch

import posenc_oracle as PO

pytestmark = pytest.mark.gpu

WIDTH = 128
PAD = 64                             # extra rows of every output
SENT = 12345.0                       # what the float outputs hold before a call
SENT_MASK = 0x5A5A5A5A5A5A5A5A
EINVAL, ERANGE = -1, -2              # include/dvgo_hip.h


# ------------------------------------------------------------------ inputs
def make_params(P, E, seed, w_scale=(1.0, 1.0, 1.0)):
    """fp32 (W1, b1, W2, b2, W3, b3) on the GPU: make_rgbnet's init plus 0.05 * randn (the `_head` of test_gpu_posenc.py),
    then layer by layer scaled by w_scale."""
    from directvoxgo_amd.dvgo import make_rgbnet
    torch.manual_seed(seed)
    net = make_rgbnet(3 + 6 * P + E, WIDTH, 3)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(torch.randn_like(p) * 0.05)
        for lin, s in zip((net[0], net[2][0], net[3]), w_scale):
            lin.weight.mul_(s)
            lin.bias.mul_(s)
    return [t.detach().cuda().contiguous() for t in (net[0].weight, net[0].bias, net[2][0].weight, net[2][0].bias,
                                                     net[3].weight, net[3].bias)]


SPECIAL = (0.0, -0.0, 1e-20, 1.5, -1.5)


def make_batch(Pm, P, E, M, seed, rays='sorted', n_rays=50, special=False):
    """dict of M tie-free rows: pts [M,3] uniform in +-1.5, freq [P], emb [N,E] (a plain random array), ray_id [M],
    g_rgb [M,3].  `special`: each of SPECIAL on each axis of eight candidate rows, and on all three axes of one."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    n = 2 * M + 64
    pts = torch.rand(n, 3, device='cuda', generator=g) * 3 - 1.5
    if special:
        r = 0
        for v in SPECIAL:
            pts[r] = v
            r += 1
            for a in range(3):
                pts[r:r + 8, a] = v
                r += 8
        assert r <= M
        pts[:M] = pts[:M][torch.randperm(M, device='cuda', generator=g)]      # among the first M: kept unless a tie
    N = n if rays == 'per_row' else n_rays
    emb = torch.rand(N, E, device='cuda', generator=g) * 2 - 1
    if rays == 'per_row':
        ray_id = torch.arange(n, device='cuda')
    elif rays == 'one':
        ray_id = torch.full((n,), N // 2, device='cuda', dtype=torch.int64)
    else:
        ray_id = torch.randint(N, (n,), device='cuda', generator=g)
        if rays == 'sorted':
            ray_id = torch.sort(ray_id)[0]
    g_rgb = torch.randn(n, 3, device='cuda', generator=g)
    freq = torch.tensor([2.0 ** i for i in range(P)], device='cuda')
    _, _, margin = PO.forward([p.double() for p in Pm], pts, freq, emb, ray_id)
    keep = PO.split_ties(margin).nonzero()[:, 0]
    assert keep.numel() >= M, f'only {keep.numel()} tie-free rows of {n}'
    keep = keep[:M]
    return dict(P=P, E=E, freq=freq, emb=emb.contiguous(), pts=pts[keep].contiguous(), ray_id=ray_id[keep].contiguous(),
                g_rgb=g_rgb[keep].contiguous())


def rows_of(b, sl):
    """The batch restricted to rows `sl` (a slice or an index tensor)."""
    return dict(b, pts=b['pts'][sl].contiguous(), ray_id=b['ray_id'][sl].contiguous(), g_rgb=b['g_rgb'][sl].contiguous())


# ------------------------------------------------------------------ the kernels through the C ABI (as shade.py calls them)
def default_n_parts(M):
    from directvoxgo_amd.shade import N_PARTS
    return max(1, min(N_PARTS, (M + 31) // 32))          # _ShadePosenc.backward


def buffers(M, d_in, n_parts):
    """Every array a kernel writes, 64 rows longer than asked for and pre-filled."""
    dev = 'cuda'
    rec = WIDTH * WIDTH + WIDTH * d_in + 5 * WIDTH + 3
    new = lambda *s: torch.full(s, SENT, device=dev)          # noqa: E731
    return dict(rgb=new(M + PAD, 3), H1=new(M + PAD, WIDTH), H2=new(M + PAD, WIDTH), G1=new(M + PAD, WIDTH), gz=new(M + PAD, 3),
                masks=torch.full((M + PAD, 4), SENT_MASK, dtype=torch.int64, device=dev),
                part=torch.full((n_parts + 1, rec), float('nan'), device=dev),
                tot=torch.full((rec + PAD,), float('nan'), device=dev))


def abi_args(Pm, b, o, **over):
    """The argument lists of the three entry points by name, in the order of include/dvgo_hip.h, for the batch `b` and
    the buffers `o`; `over` replaces arguments by name (a tensor, None for a null pointer, or an int)."""
    from directvoxgo_amd._lib import _i64, _int, ptr, stream_of
    W1, b1, W2, b2, W3, b3 = Pm
    v = dict(pts=b['pts'], freq=b['freq'], P=b['P'], emb=b['emb'], E=b['E'], ray_id=b['ray_id'], W1=W1, b1=b1, W2=W2,
             b2=b2, W3=W3, b3=b3, width=WIDTH, d_in=W1.shape[1], g_rgb=b['g_rgb'], **o)
    v.update(M=b['pts'].shape[0], n_parts=o['part'].shape[0] - 1)
    v.update(over)
    conv = lambda k: _i64(v[k]) if k == 'M' else _int(v[k]) if isinstance(v[k], int) else ptr(v[k])     # noqa: E731
    names = dict(
        dvgo_shade_pe_fwd='pts freq P emb E ray_id M W1 b1 W2 b2 W3 b3 width d_in rgb H1 H2 masks',
        dvgo_shade_pe_bwd='g_rgb rgb masks M W2 W3 width G1 gz',
        dvgo_shade_pe_wgrad='G1 gz masks W3 H1 H2 pts freq P emb E ray_id M width d_in n_parts part tot')
    return {f: [conv(k) for k in s.split()] + [stream_of(W1)] for f, s in names.items()}


def raw(name, args):
    """The entry point's return code."""
    from directvoxgo_amd import _lib as L
    return int(getattr(L.lib(), name)(*args[name]))


def unpack(o, d_in):
    k = 0
    for name, shape in (('gW2', (WIDTH, WIDTH)), ('gW1', (WIDTH, d_in)), ('gW3', (3, WIDTH)), ('gb1', (WIDTH,)),
                        ('gb2', (WIDTH,)), ('gb3', (3,))):
        n = int(np.prod(shape))
        o[name] = o['tot'][k:k + n].view(shape)
        k += n
    assert k == o['tot'].numel() - PAD


def run(Pm, b, n_parts=None, wgrad=True, train=True):
    """dict of the padded outputs rgb, H1, H2, masks, G1, gz, part, tot and views gW1 .. gb3 of tot; `M`, `n_parts`."""
    M, d_in = b['pts'].shape[0], Pm[0].shape[1]
    n_parts = default_n_parts(M) if n_parts is None else n_parts
    o = buffers(M, d_in, n_parts)
    a = abi_args(Pm, b, o, **({} if train else dict(H1=None, H2=None, masks=None)))
    assert raw('dvgo_shade_pe_fwd', a) == 0
    if train:
        assert raw('dvgo_shade_pe_bwd', a) == 0
        if wgrad:
            assert raw('dvgo_shade_pe_wgrad', a) == 0
    torch.cuda.synchronize()
    unpack(o, d_in)
    o.update(M=M, n_parts=n_parts, wgrad=wgrad and train, train=train)
    return o


def assert_untouched(o, M, n_parts_written=0, tot_written=False):
    """Rows >= M of every output, the record past the last partial and the floats past the total hold what they held."""
    for k in ('rgb', 'H1', 'H2', 'G1', 'gz'):
        assert bool((o[k][M:] == SENT).all()), f'{k} written past row {M}'
    assert bool((o['masks'][M:] == SENT_MASK).all()), f'masks written past row {M}'
    assert bool(torch.isnan(o['part'][n_parts_written:]).all()), f'part written past record {n_parts_written}'
    rec = o['tot'].numel() - PAD
    assert bool(torch.isnan(o['tot'][rec if tot_written else 0:]).all()), 'total written past its end'


_F_OF_BIT = None


def decode_masks(masks, layer):
    """[M, 128] bool from the sign-bit words [row][layer][half]: bit 16t + r of half h is feature
    32t + (r & 3) + 8(r >> 2) + 4h (pe_acc_feature)."""
    global _F_OF_BIT
    if _F_OF_BIT is None:
        bit = torch.arange(64)
        t, r = bit >> 4, bit & 15
        _F_OF_BIT = torch.stack([32 * t + (r & 3) + 8 * (r >> 2) + 4 * h for h in (0, 1)]).cuda()      # [half][bit]
        assert sorted(_F_OF_BIT.flatten().tolist()) == list(range(128))
    k = torch.zeros((masks.shape[0], WIDTH), dtype=torch.bool, device=masks.device)
    shifts = torch.arange(64, device=masks.device)
    for h in (0, 1):
        k[:, _F_OF_BIT[h]] = ((masks[:, 2 * layer + h].unsqueeze(1) >> shifts) & 1).bool()
    return k


def reference(Pm, b):
    P64 = [p.double() for p in Pm]
    args = (P64, b['pts'], b['freq'], b['emb'], b['ray_id'], b['g_rgb'])
    return PO.rows(*args) + PO.forward_backward(*args)


ROWS = (('rgb', 'rgb'), ('H1', 'h1'), ('H2', 'h2'), ('gz', 'gz'), ('G1', 'G1'))       # output -> oracle key


def check(Pm, b, got=None, ref=None, n_parts=None):
    """Hold every output of `got` (default: a fresh run) to the oracle, and the sentinels to their values."""
    got = run(Pm, b, n_parts=n_parts) if got is None else got
    row, rmag, tot, tmag = reference(Pm, b) if ref is None else ref
    M = got['M']
    assert M == b['pts'].shape[0]
    for k, r in ROWS if got['train'] else ROWS[:1]:
        PO.assert_close(k, got[k][:M], row[r], rmag[r], PO.K_ROW)
    if got['train']:
        for layer, r in ((0, 'k1'), (1, 'k2')):
            bad = decode_masks(got['masks'][:M], layer) != row[r]
            assert not bool(bad.any()), f'{int(bad.sum())} sign bits of layer {layer + 1} differ; first at {bad.nonzero()[:5].tolist()}'
    if got['wgrad']:
        for k in PO.SUM_KEYS:
            PO.assert_close(k, got[k], tot[k], tmag[k], PO.K_SUM)
    if got['train']:
        assert_untouched(got, M, got['n_parts'] if got['wgrad'] else 0, got['wgrad'])
    else:
        for k in ('H1', 'H2', 'G1', 'gz'):
            assert bool((got[k] == SENT).all()), k
        assert bool((got['rgb'][M:] == SENT).all()) and bool((got['masks'] == SENT_MASK).all())
    return got


# ------------------------------------------------------------------ input widths
SHAPES = [(1, 3), (4, 5), (4, 6), (1, 27), (4, 27), (9, 7), (9, 8), (10, 27), (15, 2), (15, 3)]


def _sid(s):
    return f'P{s[0]}-E{s[1]}-dIn{3 + 6 * s[0] + s[1]}'


@pytest.mark.parametrize('P,E', SHAPES, ids=[_sid(s) for s in SHAPES])
def test_input_widths(P, E):
    Pm = make_params(P, E, seed=100 * P + E)
    check(Pm, make_batch(Pm, P, E, 2000, seed=P + E))


# ------------------------------------------------------------------ partition edges
EDGE_M = [1, 2, 31, 32, 33, 255, 256, 257, 512, 513, 1567, 16384, 16385, 65536, 65537]


@pytest.mark.parametrize('M', EDGE_M)
@pytest.mark.parametrize('P,E', [(4, 27), (15, 2)], ids=[_sid((4, 27)), _sid((15, 2))])
def test_partition_edges(P, E, M):
    """32-row tiles, 256-row workgroups, n_parts = ceil(M / 32) = 16 / 17 / 49 and its clamp at 512, the second pass of
    the forward's and backward's grid-stride loop (65537: the largest batch in this file)."""
    Pm = make_params(P, E, seed=11)
    check(Pm, make_batch(Pm, P, E, M, seed=M))


@pytest.mark.parametrize('M', [40, 1000, 1025])
def test_n_parts_chosen_by_the_caller(M):
    """Any n_parts gives the same sums within the same bounds, also above the tile count (workgroups without a tile write
    a record of zeros) and where the reduce's slices hold 0, 1, 2 or 3 parts beside its 4-way unrolled loop."""
    P, E = 4, 27
    Pm = make_params(P, E, seed=12)
    b = make_batch(Pm, P, E, M, seed=M)
    ref = reference(Pm, b)
    for n_parts in (1, 3, 7, 16, 17, 50, 512):
        try:
            check(Pm, b, ref=ref, n_parts=n_parts)
        except AssertionError as e:
            raise AssertionError(f'n_parts = {n_parts}: {e}') from None


# ------------------------------------------------------------------ the forward every render takes
@pytest.mark.parametrize('M', [33, 2000])
def test_forward_without_activations_gives_the_same_bits(M):
    """H1 = H2 = masks = nullptr: rgb is the training forward's bit for bit, and nothing else is written."""
    P, E = 4, 27
    Pm = make_params(P, E, seed=13)
    b = make_batch(Pm, P, E, M, seed=M)
    ref = reference(Pm, b)
    train = check(Pm, b, got=run(Pm, b, wgrad=False), ref=ref)
    render = check(Pm, b, got=run(Pm, b, train=False), ref=ref)
    assert torch.equal(render['rgb'], train['rgb'])


# ------------------------------------------------------------------ position independence
def test_rows_are_position_independent():
    """A row's rgb, gz and G1 row (and its activations and sign bits) have the same bits wherever the row sits and on a
    second run.  The weight gradients meet through float atomics: they are held to the bound, not bitwise."""
    P, E = 4, 27
    Pm = make_params(P, E, seed=31)
    full = make_batch(Pm, P, E, 1000 + 33, seed=32)
    keys = ('rgb', 'gz', 'G1', 'H1', 'H2', 'masks')
    M = 1000
    base = check(Pm, rows_of(full, slice(33, None)))
    again = check(Pm, rows_of(full, slice(33, None)))
    for k in keys:
        assert torch.equal(again[k], base[k]), f'second run: {k}'
    for off in (1, 17, 33):
        o = check(Pm, rows_of(full, slice(33 - off, None)))
        for k in keys:
            assert torch.equal(o[k][off:off + M], base[k][:M]), f'offset {off}: {k}'
    perm = torch.cat([torch.arange(M // 2, M), torch.arange(M // 2)]).cuda()
    o = check(Pm, rows_of(rows_of(full, slice(33, None)), perm))
    for k in keys:
        assert torch.equal(o[k][:M], base[k][:M][perm]), f'halves swapped: {k}'


# ------------------------------------------------------------------ inputs away from the plain batch
@pytest.mark.parametrize('rays', ['sorted', 'unsorted', 'one', 'per_row'])
def test_ray_layouts(rays):
    P, E = 4, 27
    Pm = make_params(P, E, seed=51)
    check(Pm, make_batch(Pm, P, E, 3000, seed=52, rays=rays))


@pytest.mark.parametrize('P,E', [(4, 27), (15, 2)], ids=[_sid((4, 27)), _sid((15, 2))])
def test_special_positions(P, E):
    """+0, -0, 1e-20 and +-1.5 exactly, on every axis, beside random rows."""
    Pm = make_params(P, E, seed=53)
    b = make_batch(Pm, P, E, 1000, seed=54, special=True)
    bits = b['pts'].view(torch.int32)
    for v in SPECIAL:
        vb = torch.tensor([v], dtype=torch.float32).view(torch.int32).item()
        for a in range(3):
            assert bool((bits[:, a] == vb).any()), f'premise: no tie-free row has {v} on axis {a}'
    check(Pm, b)


@pytest.mark.parametrize('w_scale', [(10, 0.1, 1), (0.1, 10, 3), (3, 3, 0.1)], ids=str)
def test_trained_weight_scales(w_scale):
    P, E = 10, 27
    Pm = make_params(P, E, seed=41, w_scale=w_scale)
    check(Pm, make_batch(Pm, P, E, 3000, seed=42))


# ------------------------------------------------------------------ exactly-zero pre-activations
@pytest.mark.parametrize('P,E', [(4, 27), (4, 6)], ids=[_sid((4, 27)), _sid((4, 6))])
def test_zero_preactivations_pass_no_gradient(P, E):
    """Units whose pre-activation is exactly +0 or -0 (every term a zero: weight rows and biases of +0 / of -0), in layer 1
    and in layer 2.  relu'(0) = 0 in torch: they contribute no gradient."""
    Pm = make_params(P, E, seed=71)
    W1, b1, W2, b2, W3, b3 = Pm
    W1[3] = 0.0; b1[3] = 0.0                       # layer 1, +0
    W1[5] = -0.0; b1[5] = -0.0                     # layer 1, -0
    W2[7] = -0.0; b2[7] = -0.0                     # layer 2, -0
    W2[9] = 0.0; b2[9] = 0.0                       # layer 2, +0
    assert torch.signbit(W1[5]).all() and torch.signbit(b2[7])
    o = check(Pm, make_batch(Pm, P, E, 3000, seed=72))
    M = o['M']
    for u in (3, 5):
        assert float(o['H1'][:M, u].abs().max()) == 0 and float(o['G1'][:M, u].abs().max()) == 0, f'layer-1 unit {u}'
        assert float(o['gW1'][u].abs().max()) == 0 and float(o['gb1'][u].abs()) == 0, f'layer-1 unit {u}'
        assert float(o['gW2'][:, u].abs().max()) == 0, f'layer-1 unit {u}'
    for v in (7, 9):
        assert float(o['H2'][:M, v].abs().max()) == 0, f'layer-2 unit {v}'
        assert float(o['gW2'][v].abs().max()) == 0 and float(o['gb2'][v].abs()) == 0, f'layer-2 unit {v}'
        assert float(o['gW3'][:, v].abs().max()) == 0, f'layer-2 unit {v}'


# ------------------------------------------------------------------ non-finite positions
def test_non_finite_position_propagates():
    """One row with an inf coordinate, one with a NaN.  Their colour is finite or not where torch float32's is, and the
    weight gradients are not all finite.  Every other row is bit for bit what it is without them."""
    P, E = 4, 27
    Pm = make_params(P, E, seed=81)
    b = make_batch(Pm, P, E, 1000, seed=82)
    clean = run(Pm, b)
    bad = {100: float('inf'), 200: float('nan')}
    pts = b['pts'].clone()
    for r, v in bad.items():
        pts[r, 1] = v
    o = run(Pm, dict(b, pts=pts))
    M = o['M']
    assert_untouched(o, M, o['n_parts'], True)
    other = torch.ones(M + PAD, dtype=torch.bool, device='cuda')
    other[list(bad)] = False
    for k in ('rgb', 'gz', 'G1'):
        assert torch.equal(o[k][other], clean[k][other]), k
    W1, b1, W2, b2, W3, b3 = Pm
    arg = (pts.unsqueeze(-1) * b['freq']).flatten(-2)
    x = torch.cat([pts, arg.sin(), arg.cos(), b['emb'][b['ray_id']]], -1)
    ref = torch.sigmoid(torch.relu(torch.relu(x @ W1.t() + b1) @ W2.t() + b2) @ W3.t() + b3)
    for r in bad:
        assert not bool(torch.isfinite(ref[r]).any()), 'premise: torch gives no finite colour on the row'
        assert torch.equal(torch.isfinite(o['rgb'][r]), torch.isfinite(ref[r])), f'row {r}: rgb {o["rgb"][r].tolist()}'
    for k in PO.SUM_KEYS:
        assert not bool(torch.isfinite(o[k]).all()), f'{k} is finite: the non-finite rows vanished'


# ------------------------------------------------------------------ the empty batch
@pytest.mark.parametrize('null', [False, True], ids=['arrays', 'null-pointers'])
def test_empty_batch_at_the_abi(null):
    """M = 0: all three calls return 0 without writing a row or a partial record; the total comes back as zeros.  With
    real arrays, and with the null pointers that empty tensors have."""
    P, E = 4, 27
    Pm = make_params(P, E, seed=91)
    b = make_batch(Pm, P, E, 40, seed=92)
    o = buffers(0, Pm[0].shape[1], 4)
    over = {}
    if null:
        empty = torch.empty((0, 3), device='cuda')
        assert empty.data_ptr() == 0
        over = {k: None for k in ('pts', 'ray_id', 'g_rgb', 'rgb', 'H1', 'H2', 'masks', 'G1', 'gz', 'part')}
    a = abi_args(Pm, b, o, M=0, **over)
    for name in ('dvgo_shade_pe_fwd', 'dvgo_shade_pe_bwd', 'dvgo_shade_pe_wgrad'):
        assert raw(name, a) == 0, name
    torch.cuda.synchronize()
    assert_untouched(o, 0, 0, True)
    rec = o['tot'].numel() - PAD
    assert bool((o['tot'][:rec] == 0).all())


@pytest.mark.parametrize('deferred', [False, True], ids=['direct', 'defer_wgrad'])
def test_empty_batch_through_autograd(deferred):
    """shade_posenc on no rows: an empty rgb, and after backward six parameter gradients of zeros."""
    from directvoxgo_amd.dvgo import make_rgbnet
    from directvoxgo_amd.shade import defer_wgrad, shade_posenc
    P, E = 4, 27
    net = make_rgbnet(3 + 6 * P + E, WIDTH, 3).cuda()
    pts = torch.empty((0, 3), device='cuda')
    emb = torch.rand(5, E, device='cuda')
    rid = torch.empty((0,), dtype=torch.int64, device='cuda')
    freq = torch.tensor([2.0 ** i for i in range(P)], device='cuda')
    if deferred:
        with defer_wgrad() as d:
            rgb = shade_posenc(net, pts, emb, rid, freq)
            rgb.backward(torch.empty_like(rgb))
        d.flush()
    else:
        rgb = shade_posenc(net, pts, emb, rid, freq)
        rgb.backward(torch.empty_like(rgb))
    torch.cuda.synchronize()
    assert rgb.shape == (0, 3) and rgb.requires_grad
    for name, p in net.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, name
        assert bool((p.grad == 0).all()), name


# ------------------------------------------------------------------ argument checks
def test_return_codes_without_a_launch():
    """What the entry points refuse, they refuse before touching a buffer."""
    P, E, M, n_parts = 4, 27, 100, 4
    Pm = make_params(P, E, seed=95)
    b = make_batch(Pm, P, E, M, seed=96)
    d_in = 3 + 6 * P + E
    o = buffers(M, d_in, n_parts)
    F, B, W = 'dvgo_shade_pe_fwd', 'dvgo_shade_pe_bwd', 'dvgo_shade_pe_wgrad'
    cases = [
        ('width 64', dict(width=64), ERANGE, (F, B, W)),
        ('P = 0', dict(P=0, d_in=3 + E), ERANGE, (F, W)),
        ('P = 16', dict(P=16, d_in=3 + 96 + E), ERANGE, (F, W)),
        ('P = 16, E = 0', dict(P=16, E=0, d_in=99), ERANGE, (F, W)),
        ('d_in != 3 + 6P + E', dict(d_in=d_in + 1), ERANGE, (F, W)),
        ('d_in != 3 + 6P + E', dict(d_in=d_in - 1), ERANGE, (F, W)),
        ('d_in = 97', dict(P=15, E=4, d_in=97), ERANGE, (F, W)),
        ('d_in = 102', dict(P=12, E=27, d_in=102), ERANGE, (F, W)),
        ('M < 0', dict(M=-1), EINVAL, (F, B, W)),
        ('n_parts = 0', dict(n_parts=0), EINVAL, (W,)),
        ('n_parts < 0', dict(n_parts=-3), EINVAL, (W,)),
        ('H1 null, H2 given', dict(H1=None), EINVAL, (F,)),
    ]
    for what, over, rc, names in cases:
        a = abi_args(Pm, b, o, **over)
        for name in names:
            assert raw(name, a) == rc, f'{name}: {what}'
        torch.cuda.synchronize()
        assert_untouched(o, 0, 0, False)
