"""GPU: the brick scatter (csrc/brick.hip) and the Adam update fused into it, elementwise against the float64 statement
of tests/brick_oracle.py (derivation of every bound there; tests/test_brick_oracle_host.py pins the statement itself).

Every comparison is per voxel and channel: |got - ref| <= gamma(n + S + 1) * mag with the voxel's own n and mag, exact
zeros where nothing contributes, and for the update m, v and p of every element tied to the same float64 gradient.
  * model scenes through `LaunchSpy`: the oracle runs on the kernel's actual arguments, inside TrainStep too;
  * synthetic lists at the library boundary: list lengths at the chunk and slice edges, an exactly full reference table,
    records without features, partial bricks, xyz_max, C in {3, 4, 9, 12} x modes {0, 1, 2 then 3}, unmasked flags;
  * the two 160^3 scenes, mode 0 and one fused step;
  * the paths no in-process test reached: TAIL_SCANS, bricks without heavy-brick tables.
The undetermined counts (elements whose float64 gradient is within the bound of zero) are printed by every Adam check and
capped at 1e-4 of the elements with a contribution.

What the file sees.  Four value-only faults were put into brick.hip, one at a time, in builds kept aside; the tests that
failed (names as of that run; `old` = tests/test_gpu_brick.py):
  adam4 leaves m.y unchanged at voxels whose index is a multiple of 1024
      old  adam_fused_into_the_brick_kernel_equals_dense_gradients_plus_masked_adam (both), heavy_bricks_are_split_...
      new  model_scene_fused_adam_... [20-12] [23-12], sync_free_step_..., thin_slab_heavy_bricks, tail_scans_...,
           bricks_without_heavy_brick_tables, synthetic_lists_fused_adam [*-12], synthetic_two_ranks_... [*-12], both 160^3
  the sort writes weight 0 for corner 7 when its weight is below 1e-3
      old  brick_gradients_match_oracle_scatter (all four), scatter_variants_agree_at_full_size, dedup_table_overflow_...,
           heavy_bricks_are_split_...
      new  every model-scene test (dense and fused Adam, every lattice), sync_free_step_..., scattered_samples_scene,
           thin_slab_heavy_bricks, tail_scans_..., bricks_without_heavy_brick_tables, both 160^3; no synthetic test (their
           weights are >= 1e-3 by construction)
  the meeting loop of a heavy brick skips the last slice
      old  brick_gradients_match_oracle_scatter [20-12] [23-12] [26-9], scatter_variants_agree_at_full_size, adam_fused_... (both),
           heavy_bricks_are_split_...
      new  model-scene dense and fused Adam at 20^3, 23^3, 26^3, sync_free_step_..., thin_slab_heavy_bricks, tail_scans_...,
           every synthetic test (dense, fused Adam, two ranks; every family and C), roofline 160^3
  the C == 12 masked test looks at g.x only
      old  none
      new  synthetic_lists_fused_adam [*-12] and synthetic_two_ranks_... [*-12] only: no model scene and neither 160^3 scene
           has a float4 with g.x exactly zero beside a non-zero lane, so only the hand-made lists, whose bricks carry an
           exactly-zero lane in every float4 (brick_oracle.synthetic), see a float4-wide masked test.
"""
import numpy as np
import pytest
import torch

import brick_oracle as B
from test_gpu_brick import _grads, _model

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ model scenes
def _toggle(variant):
    from directvoxgo_amd import _lib as L, fused as F
    from directvoxgo_amd._lib import _int
    F.BRICK_SCATTER = variant == 'brick'
    F.COMBINED_GRID_GRAD, F.COMBINED_MIN_RATIO = (variant == 'rows', 1e9) if variant != 'brick' else (True, 6)
    for knob in (0, 1):
        L.call('dvgo_set_tuning', _int(knob), _int(0 if variant == 'naive' else 1))


def _march_backward(m, sc, variant, stepsize=None, seed=11):
    """fused_march + backward of seeded random output gradients (the same for every variant) -> density.grad, k0.grad"""
    from directvoxgo_amd import fused as F
    cfg = m._march_cfg(sc['near'], sc['far'], stepsize or sc['stepsize'])
    _toggle(variant)
    try:
        m.zero_grad(set_to_none=True)
        w, alpha, last, feat, ray_id, step_id, off3 = F.fused_march(m.density, m.k0, sc['rays_o'], sc['rays_d'], cfg)
        gen = torch.Generator(device='cuda').manual_seed(seed)
        gs = [torch.randn(t.shape, device='cuda', generator=gen) for t in (w, last, feat)]
        torch.autograd.backward([w, last, feat], gs)
        torch.cuda.synchronize()
        return m.density.grad.detach().cpu().numpy(), m.k0.grad.detach().cpu().numpy()
    finally:
        _toggle('brick')


def _dense_and_atomics(m, sc, variants, stepsize=None, loss=True):
    with B.LaunchSpy() as spy:
        _march_backward(m, sc, 'brick', stepsize)
        if loss:
            _grads(m, sc, 'brick', stepsize)                   # g_feat and the density gradient of a real loss
    assert [l.kind for l in spy.launches] == ['dense'] * (2 if loss else 1)
    O = spy.launches[0].sums
    assert (O.mag > 0).sum() > 1000 and (O.mag == 0).sum() > 0
    print('brick worst err/bound', [round(l.worst, 4) for l in spy.launches], 'max n', int(O.n.max()), 'max S', int(O.S.max()))
    for variant in variants:
        gd, gk = _march_backward(m, sc, variant, stepsize)
        print(variant, 'worst err/bound', round(B.check_dense(O, gk, gd, atomic=True, what=variant), 4))
    return spy


def _train_steps(m, sc, n=3, **kw):
    from directvoxgo_amd.train import FINE_TRAIN, TrainStep
    step = TrainStep(m, dict(FINE_TRAIN), dict(near=sc['near'], far=sc['far'], bg=1, stepsize=sc['stepsize']), **kw)
    with B.LaunchSpy() as spy:
        for it in range(n):
            step(sc['rays_o'], sc['rays_d'], sc['viewdirs'], sc['target'], global_step=5000 + it)
        torch.cuda.synchronize()
        assert [l.kind for l in spy.launches] == ['adam'] * n and step.last_fused_adam
        assert m.density.grad is None and m.k0.grad is None
        for it, l in enumerate(spy.launches):
            assert l.hyper.masked_k and l.hyper.masked_d and not l.ss_from_device
            assert (np.any(l.before[1] != 0) and np.any(l.before[2] != 0)) == (it > 0)      # steps 2, 3: non-zero moments
        # device-side step sizes (captured steps read them): one eager step after hyper_begin, nothing captured
        from directvoxgo_amd.masked_adam import adam_step_size
        step.optimizer.hyper_begin(m.density, m.k0)
        want_ss = adam_step_size(step.optimizer._group_of(m.k0)['lr'], 0.9, 0.99, n + 1)
        step(sc['rays_o'], sc['rays_d'], sc['viewdirs'], sc['target'], global_step=5000 + n)
        torch.cuda.synchronize()
        assert len(spy.launches) == n + 1 and spy.launches[-1].ss_from_device
        assert spy.launches[-1].hyper.ss_k == float(np.float32(want_ss))
    for l in spy.launches:
        print('adam', l.adam)
    return spy


SCENES = [(20, 12), (23, 12), (17, 3), (26, 9), (20, 4)]


@pytest.mark.parametrize('world,C', SCENES)
def test_model_scene_dense_gradients_of_every_scatter_variant(world, C):
    sc, m = _model(world, 700, C=C)
    assert m.k0.shape[1] == C and m.k0.stride()[1] == 1
    _dense_and_atomics(m, sc, ('naive', 'dedup') + (('rows',) if C == 12 else ()))


@pytest.mark.parametrize('world,C', SCENES)
def test_model_scene_fused_adam_three_steps_and_device_step_sizes(world, C):
    sc, m = _model(world, 700, C=C)
    _train_steps(m, sc)


def test_sync_free_step_reads_a_padded_record_buffer():
    sc, m = _model(23, 700, width=128, direct=True)
    from directvoxgo_amd.train import FINE_TRAIN, TrainStep
    step = TrainStep(m, dict(FINE_TRAIN), dict(near=sc['near'], far=sc['far'], bg=1, stepsize=sc['stepsize']), sync_free=True)
    with B.LaunchSpy() as spy:
        for it in range(2):
            step(sc['rays_o'], sc['rays_d'], sc['viewdirs'], sc['target'], global_step=5000 + it)
        torch.cuda.synchronize()
    assert [l.kind for l in spy.launches] == ['adam'] * 2
    assert spy.launches[0].n_rec_rows > spy.launches[0].inputs['off'][-1]          # padded: more rows than entries
    print('adam', [l.adam for l in spy.launches])


def test_scattered_samples_scene():
    """Steps of ~3.7 voxels: single-sample runs, most samples straddle brick faces (test_gpu_brick.py's scene)."""
    sc, m = _model(64, 4096, stepsize=3.7)
    _dense_and_atomics(m, sc, ('naive', 'dedup', 'rows'), stepsize=3.7)
    _train_steps(m, sc, n=2)


def test_thin_slab_heavy_bricks(monkeypatch):
    """A 6-voxel slab crossed by 16384 rays, slices of 1024: bricks of many slices meet in scratch tiles."""
    from directvoxgo_amd import fused as F
    monkeypatch.setattr(F, 'BRICK_SLICE', 1024)
    sc, m = _model(48, 16384, width=128, direct=True)
    with torch.no_grad():
        d = torch.full_like(m.density, -20.0)
        d[:, :, 20:26] = 6.0
        m.density.copy_(d)
        m.mask_cache.mask.fill_(True)
    spy = _dense_and_atomics(m, sc, ('naive', 'dedup', 'rows'))
    assert spy.launches[0].sums.S.max() > 2
    spy = _train_steps(m, sc, n=2)
    assert spy.launches[0].sums.S.max() > 2


# ------------------------------------------------------------------------------------------ the paths of 6a5dea8
def test_tail_scans_build_the_same_tables():
    """fused.TAIL_SCANS: the last workgroup of march_density builds the per-ray offsets and the brick tables, and no scan
    launch is issued between it and the gather.  Partial bricks (23^3)."""
    from directvoxgo_amd import fused as F
    sc, m = _model(23, 700)
    with B.LaunchSpy(check=False) as ref:
        _march_backward(m, sc, 'brick')
    assert 'dvgo_march_scans' in ref.calls
    F.TAIL_SCANS = True
    try:
        spy = _dense_and_atomics(m, sc, (), loss=False)
        adam = _train_steps(m, sc, n=1)
    finally:
        F.TAIL_SCANS = False
    for s in (spy, adam):                                     # the tail path was taken: the tables came from no scan launch
        assert 'dvgo_march_density' in s.calls and not {'dvgo_march_scans', 'dvgo_brick_scan', 'dvgo_exclusive_scan_i32'} & set(s.calls)
    # the same tables as the scan launch builds (the order inside a list is the fill's, not the scan's: sums may differ
    # in their last bits, and both were held to the oracle above)
    assert np.array_equal(spy.launches[0].inputs['off'], ref.launches[0].inputs['off'])
    assert np.array_equal(spy.launches[0].sums.n, ref.launches[0].sums.n)


def test_bricks_without_heavy_brick_tables(monkeypatch):
    """BRICK_SLICE = 1 with a record capacity >= 32768 makes _BrickPlan leave the heavy-brick tables out (the value never
    reaches a kernel): every brick runs as one workgroup, `active` is NULL and mode 1 walks all bricks."""
    from directvoxgo_amd import fused as F
    monkeypatch.setattr(F, 'BRICK_SLICE', 1)               # 8 * cap // 1 >= 2^18: _BrickPlan leaves the tables out
    sc, m = _model(23, 700)
    cfg = m._march_cfg(sc['near'], sc['far'], sc['stepsize'])
    feat = F.fused_march(m.density, m.k0, sc['rays_o'], sc['rays_d'], cfg)[3]
    plan = feat.grad_fn.plan
    assert plan.n_bricks > 0 and plan.extra_off is None and plan.active is None and plan.slice_len == 0
    spy = _dense_and_atomics(m, sc, (), loss=False)
    assert spy.launches[0].inputs['slice_len'] == 0 and spy.launches[0].sums.S.max() == 1
    _train_steps(m, sc, n=2)


# ------------------------------------------------------------------------------------------ synthetic lists
def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda', dtype=dtype)


def _tables(counts, slice_len):
    """dvgo_brick_scan on hand-made counts; the tables are checked on the host before anything is launched from them."""
    from directvoxgo_amd import _lib as L
    nb = counts.shape[0]
    cnt = _dev(counts, torch.int32)
    tabs = torch.full((3, nb + 1), -1, dtype=torch.int32, device='cuda')
    cursor = torch.empty(nb, dtype=torch.int32, device='cuda')
    st = L.stream_of(cnt)
    T = dict(off=tabs[0], extra_off=None, active=None, extra_brick=None, arrive=None, n_extra=0, slice_len=0)
    if slice_len:
        n_extra = int(counts.sum()) // slice_len
        extra_brick = torch.full((max(n_extra, 1),), -1, dtype=torch.int32, device='cuda')
        L.call('dvgo_brick_scan', cnt, nb, tabs[0], cursor, tabs[1], tabs[2], extra_brick, n_extra, slice_len, st)
        T.update(extra_off=tabs[1], active=tabs[2], extra_brick=extra_brick, arrive=cnt, n_extra=n_extra, slice_len=slice_len)
    else:
        L.call('dvgo_brick_scan', cnt, nb, tabs[0], cursor, None, None, None, 0, 0, st)
    torch.cuda.synchronize()
    off = tabs[0].cpu().numpy()
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(counts)])) and np.array_equal(cursor.cpu().numpy(), off[:-1])
    if slice_len:
        slices = np.where(counts > slice_len, -(-counts // slice_len), 1)
        ex, act, eb = tabs[1].cpu().numpy(), tabs[2].cpu().numpy(), extra_brick.cpu().numpy()
        assert np.array_equal(ex, np.concatenate([[0], np.cumsum(slices - 1)])) and ex[-1] <= n_extra
        assert act[-1] == (counts > 0).sum() and np.array_equal(act[:act[-1]], np.nonzero(counts)[0])
        assert np.array_equal(eb[:ex[-1]], np.repeat(np.arange(nb), slices - 1))
        assert np.all(cnt.cpu().numpy() == 0)                                    # the arrival counters
    return T


def _k0_like(C, dims, fill):
    return torch.full((1,) + tuple(dims) + (C,), fill, dtype=torch.float32, device='cuda').permute(0, 4, 1, 2, 3)


def _accumulate(ins, T, grads=(None, None), adam=None, tiles=None, mode=0, active=None, lists=True):
    from directvoxgo_amd import _lib as L
    from directvoxgo_amd.fused import _NO_ADAM
    C, dims = ins['C'], (ins['X'], ins['Y'], ins['Z'])
    TS = (C + 4) // 4 * 4
    scratch = torch.empty((2 * T['n_extra'] + 1, 512 * TS), dtype=torch.float32, device='cuda') if T['slice_len'] else None
    keep = [_dev(ins[k]) for k in ('recs', 'rays_start', 'rays_dir', 'grad_feat')] if lists else [None] * 4
    assert not lists or (keep[0].shape[0] >= int(T['off'][-1]) and keep[3].data_ptr() % 16 == 0)
    a = dict(brick_off=T['off'], extra_off=T['extra_off'], active=active if active is not None else T['active'],
             extra_brick=T['extra_brick'], arrive=T['arrive'], scratch=scratch, n_extra_max=T['n_extra'], slice_len=T['slice_len'],
             recs=keep[0], rays_start=keep[1], rays_dir=keep[2], stepdist=float(ins['stepdist']), xyz_min=L.f3(ins['xyz_min']),
             xyz_max=L.f3(ins['xyz_max']), grad_feat=keep[3], C=C, X=dims[0], Y=dims[1], Z=dims[2], grad_k0=grads[0],
             grad_density=grads[1], tiles=tiles, tiles_mode=mode, stream=L.stream_of(T['off']))
    a.update(zip(B._ADAM_RUN, adam or _NO_ADAM))
    index = B.param_index('dvgo_brick_accumulate')           # arguments by the header's names, in the header's order
    assert set(index) == set(a)
    L.call('dvgo_brick_accumulate', *[a[k] for k in sorted(index, key=index.get)])
    torch.cuda.synchronize()


def _adam_state(C, dims, seed, masked=(1, 1)):
    g = torch.Generator(device='cuda').manual_seed(seed)
    r = lambda shape, scale: torch.randn(shape, device='cuda', generator=g) * scale
    pk, mk = _k0_like(C, dims, 0).add_(r((1, C) + tuple(dims), 1.0)), _k0_like(C, dims, 0).add_(r((1, C) + tuple(dims), 0.1))
    vk = _k0_like(C, dims, 0).add_(r((1, C) + tuple(dims), 0.1).square())
    pd, md = r((1, 1) + tuple(dims), 1.0), r((1, 1) + tuple(dims), 0.1)
    vd = r((1, 1) + tuple(dims), 0.1).square()
    assert pk.stride()[1] == 1 and mk.stride() == pk.stride() and vk.stride() == pk.stride()
    H = B.Hyper(0.1, masked[0], 0.07, masked[1], 0.9, 0.99, 1e-8)
    grids = [pk, mk, vk, pd, md, vd]
    args = (pk, mk, vk, 0.1, masked[0], pd, md, vd, 0.07, masked[1], 0.9, 0.99, 1e-8, None)
    return grids, args, H


def _host(grids):
    return [t.detach().cpu().numpy().copy() for t in grids]


@pytest.mark.parametrize('C', [3, 4, 9, 12])
@pytest.mark.parametrize('family', B.SYN_FAMILIES)
def test_synthetic_lists_dense_gradients(C, family):
    """Mode 0: list lengths 1 .. 3 * slice + 7, 2048 references in one chunk, corner-only records, records without features,
    partial bricks, xyz_max; slices of one chunk (256) and of four (1024), and the longer lists without heavy-brick tables."""
    for spec_slice, slice_len in ((256, 256), (1024, 1024), (1024, 0)):
        ins, counts = B.synthetic_case(family, C, 'A', spec_slice)
        dims = (ins['X'], ins['Y'], ins['Z'])
        O = B.scatter(**ins, slice_len=slice_len)
        gk, gd = _k0_like(C, dims, float('nan')), torch.full((1, 1) + dims, float('nan'), device='cuda')
        _accumulate(ins, _tables(counts, slice_len), grads=(gk, gd))
        print(family, C, slice_len, 'worst err/bound', round(B.check_dense(O, gk.cpu().numpy(), gd.cpu().numpy()), 4), 'max n', int(O.n.max()))


@pytest.mark.parametrize('C', [3, 4, 9, 12])
@pytest.mark.parametrize('family', B.SYN_FAMILIES)
def test_synthetic_lists_fused_adam(C, family):
    """Mode 1 from non-zero moments: masked (what TrainStep issues), then the unmasked flags with their documented meaning
    (plain Adam on every voxel of a listed brick, nothing elsewhere), then one of each."""
    for masked, spec_slice, slice_len in (((1, 1), 256, 256), ((1, 1), 1024, 1024), ((1, 1), 1024, 0), ((0, 0), 1024, 1024),
                                          ((1, 0), 256, 256), ((0, 1), 256, 0)):
        ins, counts = B.synthetic_case(family, C, 'A', spec_slice)
        dims = (ins['X'], ins['Y'], ins['Z'])
        O = B.scatter(**ins, slice_len=slice_len)
        grids, args, H = _adam_state(C, dims, seed=C, masked=masked)
        before = _host(grids)
        _accumulate(ins, _tables(counts, slice_len), adam=args)
        print(family, C, masked, slice_len, B.check_adam(O, before, _host(grids), H))


@pytest.mark.parametrize('C', [3, 4, 9, 12])
@pytest.mark.parametrize('family', B.SYN_FAMILIES)
@pytest.mark.parametrize('sl', B.SYN_SLICES)
def test_synthetic_two_ranks_tiles_out_then_tiles_in(C, family, sl):
    """Modes 2 then 3: two different lists stand in for two ranks; the union table comes from dvgo_brick_scan on the summed
    counts, the tiles are added on the device, and the oracle is Adam on the float64 sum of both lists.  One brick only
    rank B touches, many only rank A touches, and a brick heavy on both (mode 2's binary search for its tile)."""
    from directvoxgo_amd import _lib as L
    A, cA = B.synthetic_case(family, C, 'A', sl)
    Bq, cB = B.synthetic_case(family, C, 'B', sl)
    dims = (A['X'], A['Y'], A['Z'])
    nb = cA.shape[0]
    O = B.scatter(**A, slice_len=sl) + B.scatter(**Bq, slice_len=sl)
    union_cnt = _dev(cA + cB, torch.int32)
    tabs = torch.full((4, nb + 1), -1, dtype=torch.int32, device='cuda')
    L.call('dvgo_brick_scan', union_cnt, nb, tabs[0], tabs[1], tabs[2], tabs[3], tabs[1], 0, 1 << 30, L.stream_of(tabs))
    torch.cuda.synchronize()
    act = tabs[3].cpu().numpy()
    n_union = int(act[-1])
    assert n_union == ((cA + cB) > 0).sum() and np.array_equal(act[:n_union], np.nonzero(cA + cB)[0])
    TS = (C + 4) // 4 * 4
    tiles = []
    for ins, counts in ((A, cA), (Bq, cB)):
        T = _tables(counts, sl)
        assert T['extra_off'][-1] > 0                                            # both ranks have a sliced brick
        t = torch.full((n_union, 512 * TS), float('nan'), device='cuda')
        _accumulate(ins, T, tiles=t, mode=2, active=tabs[3])
        tiles.append(t)
    summed = tiles[0] + tiles[1]
    assert bool(torch.isfinite(summed).all())                                     # every listed tile was written by both
    grids, args, H = _adam_state(C, dims, seed=100 + C)
    before = _host(grids)
    _accumulate(A, _tables(cA, sl), adam=args, tiles=summed, mode=3, active=tabs[3], lists=False)
    print(family, C, sl, B.check_adam(O, before, _host(grids), H))


# ------------------------------------------------------------------------------------------ full size
def _full_size(sc, m):
    import time
    rk = dict(near=sc['near'], far=sc['far'], bg=1, stepsize=sc['stepsize'])
    t0 = time.time()
    with B.LaunchSpy() as spy:
        _march_backward(m, sc, 'brick')
    assert spy.launches[0].kind == 'dense'
    O = spy.launches[0].sums
    print('dense worst err/bound', round(spy.launches[0].worst, 4), 'entries', int(spy.launches[0].inputs['off'][-1]),
          'max n', int(O.n.max()), 'max S', int(O.S.max()), 'oracle + check seconds', round(time.time() - t0, 1))
    del spy, O
    from directvoxgo_amd.train import FINE_TRAIN, TrainStep
    step = TrainStep(m, dict(FINE_TRAIN), rk)
    t0 = time.time()
    with B.LaunchSpy() as spy:
        step(sc['rays_o'], sc['rays_d'], sc['viewdirs'], sc['target'], global_step=5000)
        torch.cuda.synchronize()
    assert [l.kind for l in spy.launches] == ['adam']
    print('adam', spy.launches[0].adam, 'seconds', round(time.time() - t0, 1))


@pytest.mark.timeout(600)
def test_roofline_160_cubed_elementwise():
    """160^3 x 12, 8192 rays x 256 samples, every sample kept: mode 0 and one fused Adam step, every voxel and channel
    (no brick is subsampled).  Measured: 2 970 370 list entries; oracle + check 3.4 s for the dense gradients and 7.1 s for
    the step (np.bincount per channel; the Adam check walks the voxels half a million at a time)."""
    sc, m = _model(160, 8192, width=128, direct=True, scene='roofline')
    _full_size(sc, m)


@pytest.mark.timeout(600)
def test_lego_like_160_cubed_elementwise():
    """The lego-like 160^3 scene (mask, both filters, early stop): mode 0 and one fused Adam step, every voxel and channel.
    Measured: 307 779 list entries; oracle + check 1.4 s and 4.8 s."""
    sc, m = _model(160, 8192, width=128, direct=True)
    _full_size(sc, m)
