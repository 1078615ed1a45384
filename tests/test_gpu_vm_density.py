"""GPU: the vector-matrix density (csrc/vm_density.hip) against the float64 oracle of tests/vm_density_oracle.py on every
sample, texel and line node; against `vm_sample(...).sum(-1)`; its zero-gradient rule; the op's autograd against a float64
torch restatement; and `TensoRFVoxGO.dense_density()` at the lattice.

Error bounds (U = 2^-24; A = the magnitude the oracle returns), derived, not tuned:
  forward   |got - ref| <= (3R + 12) U A.  Each product carries 12 U A_j (tests/test_gpu_vm.py's derivation); the 3R - 1
            additions each round a partial sum of magnitude at most A, in any order (an fma chain rounds fewer times);
            rounded up by one.
  backward  |got - ref| <= (n + 12) U A per texel and per line node with n contributions: tests/test_gpu_vm.py's bound,
            whose terms are the same with one fewer distinct factor.
No element is excluded from either check.
"""
import numpy as np
import pytest
import torch

import vm_density_cases as C
import vm_density_oracle as DO
import vm_oracle as VO

pytestmark = pytest.mark.gpu

MN, MX = C.MN, C.MX
MODES = (1, 2)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def lay_out(p, layout):
    """numpy [1,C,H,W] -> a device tensor of that shape: channel-first ('cf'), channels-last ('cl'), or a channels-last
    view that starts one float off a 16-byte boundary ('off')."""
    t = cu(p)
    if layout == 'cf':
        return t
    if layout == 'cl':
        return t.contiguous(memory_format=torch.channels_last)
    _, Cn, H, W = t.shape
    buf = torch.zeros(t.numel() + 1, device='cuda')
    assert buf.data_ptr() % 16 == 0
    view = buf[1:].as_strided((1, Cn, H, W), (H * W * Cn, 1, W * Cn, Cn))
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


def check_grads(gp, gl, rp, rl, tag, scale=1):
    """Six device buffers against `scale` times the oracle with scale * n contributions; -> worst err / bound."""
    worst = 0.0
    for k in VO.KEYS:
        for name, dev, (g, Ag, n) in (('plane', gp[k][0], rp[k]), ('line', gl[k][0, :, :, 0], rl[k])):
            gg = dev.cpu().numpy().astype(np.float64)
            err, bound = np.abs(gg - scale * g), (scale * n[None] + 12) * VO.U * scale * Ag
            if err.size:
                worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), (tag, k, name, float((err - bound).max()))
            assert (gg[:, n == 0] == 0).all(), (tag, k, name)
    return worst


def zeros_like_case(planes, lines, layout):
    return ({k: lay_out(np.zeros_like(p), layout) for k, p in planes.items()},
            {k: lay_out(np.zeros_like(p), layout) for k, p in lines.items()})


@pytest.mark.parametrize('layout', ['cf', 'cl', 'off'])
@pytest.mark.parametrize('R', C.RS)
def test_kernels_against_oracle(R, layout):
    """R = 1 and 3 take the scalar and (cf) sample-fastest branches, 4 and 8 in 'cl' the vector ones; 'off' is channels-last
    but misaligned: scalar loads, component-fastest scatter.  The forward is bitwise repeatable and, its order being one
    fma chain whatever the loads, gives the same bits in every layout."""
    from directvoxgo_amd.ops import vm_density_bwd, vm_density_fwd
    planes, lines, per_m = C.case(R)
    dp = {k: lay_out(p, layout) for k, p in planes.items()}
    dl = {k: lay_out(p, layout) for k, p in lines.items()}
    cfp = {k: cu(p) for k, p in planes.items()}
    cfl = {k: cu(p) for k, p in lines.items()}
    mn, mx = cu(MN), cu(MX)
    worst_f = worst_b = 0.0
    for M in C.MS:
        xyz, val, A, gout, (rp, rl) = per_m[M]
        dx = cu(xyz).reshape(M, 3)
        got_t = vm_density_fwd(dp, dl, dx, mn, mx)
        got = got_t.cpu().numpy().astype(np.float64)
        assert got.shape == val.shape == (M,)
        err, bound = np.abs(got - val), DO.forward_bound(R, A)
        if M:
            worst_f = max(worst_f, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (M, float((err - bound).max()))
        assert torch.equal(got_t, vm_density_fwd(dp, dl, dx, mn, mx))             # bitwise repeatable
        assert torch.equal(got_t, vm_density_fwd(cfp, cfl, dx, mn, mx))           # the order does not depend on the layout
        for mode in MODES:
            for run in (1, 4, 7):
                gp, gl = zeros_like_case(planes, lines, layout)
                vm_density_bwd(cu(gout), dp, dl, gp, gl, dx, mn, mx, run=run, mode=mode)
                worst_b = max(worst_b, check_grads(gp, gl, rp, rl, (M, mode, run)))
    print(f'R={R} {layout}: worst forward err / bound {worst_f:.3f}, worst backward err / bound {worst_b:.3f}')


@pytest.mark.parametrize('layout', ['cf', 'cl'])
def test_density_against_the_sum_of_the_sampler(layout):
    """`vm_density` against `vm_sample(...).sum(-1)` (torch's float32 row sum, an order of its own): both lie within the
    forward bound of the oracle, so they differ by at most twice the bound."""
    from directvoxgo_amd.ops import vm_density, vm_sample
    R = 8
    planes, lines, per_m = C.case(R)
    xyz, val, A = per_m[1000][:3]
    dp = {k: lay_out(p, layout) for k, p in planes.items()}
    dl = {k: lay_out(p, layout) for k, p in lines.items()}
    a = vm_density(dp, dl, cu(xyz), cu(MN), cu(MX)).cpu().numpy().astype(np.float64)
    b = vm_sample(dp, dl, cu(xyz), cu(MN), cu(MX)).sum(-1).cpu().numpy().astype(np.float64)
    bound = DO.forward_bound(R, A)
    assert (np.abs(a - val) <= bound).all() and (np.abs(b - val) <= bound).all() and np.abs(a).sum() > 0
    shaped = vm_density(dp, dl, cu(xyz).reshape(10, 100, 3), cu(MN), cu(MX))
    assert shaped.shape == (10, 100) and np.array_equal(shaped.reshape(-1).cpu().numpy().astype(np.float64), a)


def test_backward_past_the_grid_cap():
    """Mode 2 launches at most 1024 workgroups: 12 000 samples of R = 8 at run 1 are 288 000 lanes, 1125 workgroups' worth
    (a share is then two workgroup sizes); run 4 stays below the cap.  Same bound, both modes."""
    from directvoxgo_amd.ops import vm_density_bwd
    planes, lines, _ = C.case(8)
    rng = np.random.default_rng(77)
    M = 12000
    xyz = C.points(M, rng)
    gout = rng.standard_normal(M).astype(np.float32)
    rp, rl = DO.backward(planes, lines, xyz, MN, MX, gout)
    dp = {k: lay_out(p, 'cl') for k, p in planes.items()}
    dl = {k: lay_out(p, 'cl') for k, p in lines.items()}
    for mode in MODES:
        for run in (1, 4):
            gp, gl = zeros_like_case(planes, lines, 'cl')
            vm_density_bwd(cu(gout), dp, dl, gp, gl, cu(xyz), cu(MN), cu(MX), run=run, mode=mode)
            check_grads(gp, gl, rp, rl, (mode, run))


@pytest.mark.parametrize('layout', ['cf', 'cl'])
def test_backward_with_mostly_zero_gradients(layout):
    """About 80 % of grad_out exactly 0 (both signs of zero), as the alpha and weight filters leave it, against the oracle
    with the same bound.  The oracle is run on the samples with a non-zero gradient: the sums are those of all samples
    (checked), and n then counts the contributions the kernel may make, so that a cell reached only by zero-gradient
    samples must be exactly 0."""
    from directvoxgo_amd.ops import vm_density_bwd
    R = 4
    planes, lines, per_m = C.case(R)
    xyz = per_m[1000][0]
    rng = np.random.default_rng(9)
    gout = rng.standard_normal(1000).astype(np.float32)
    dead = rng.random(1000) < 0.8
    gout[dead] = np.where(rng.random(int(dead.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
    assert 0.75 < dead.mean() < 0.85 and (gout[~dead] != 0).all()
    rp, rl = DO.backward(planes, lines, xyz[~dead], MN, MX, gout[~dead])
    fp, fl = DO.backward(planes, lines, xyz, MN, MX, gout)
    for k in VO.KEYS:
        assert np.allclose(rp[k][0], fp[k][0], rtol=1e-12, atol=0) and np.allclose(rl[k][0], fl[k][0], rtol=1e-12, atol=0)
        assert (rp[k][2] <= fp[k][2]).all() and (rp[k][2] < fp[k][2]).any()
    dp = {k: lay_out(p, layout) for k, p in planes.items()}
    dl = {k: lay_out(p, layout) for k, p in lines.items()}
    for mode in MODES:
        for run in (1, 4, 7):
            gp, gl = zeros_like_case(planes, lines, layout)
            vm_density_bwd(cu(gout), dp, dl, gp, gl, cu(xyz), cu(MN), cu(MX), run=run, mode=mode)
            check_grads(gp, gl, rp, rl, (mode, run))
    gp, gl = zeros_like_case(planes, lines, layout)                               # all zero: nothing is written at all
    vm_density_bwd(cu(np.zeros(1000, np.float32)), dp, dl, gp, gl, cu(xyz), cu(MN), cu(MX))
    assert all(float(t.abs().sum()) == 0 for t in list(gp.values()) + list(gl.values()))


def test_two_backward_calls_accumulate():
    """Two calls into the same buffers against twice the oracle with 2 n contributions."""
    from directvoxgo_amd.ops import vm_density_bwd
    planes, lines, per_m = C.case(4)
    xyz, _, _, gout, (rp, rl) = per_m[1000]
    dp = {k: lay_out(p, 'cl') for k, p in planes.items()}
    dl = {k: lay_out(p, 'cl') for k, p in lines.items()}
    for mode in (0,) + MODES:
        gp, gl = zeros_like_case(planes, lines, 'cl')
        for _ in range(2):
            vm_density_bwd(cu(gout), dp, dl, gp, gl, cu(xyz), cu(MN), cu(MX), mode=mode)
        check_grads(gp, gl, rp, rl, mode, scale=2)


@pytest.mark.parametrize('wants', ['both', 'planes', 'lines'])
@pytest.mark.parametrize('layout', ['cf', 'cl'])
def test_op_autograd_against_the_float64_restatement(layout, wants):
    """ops.vm_density against the row sum of six float64 F.grid_sample and products on the CPU, on the dyadic case: values
    rtol 1e-5 / atol 1e-6, gradients rtol 1e-4 / atol 1e-6.  With only the planes or only the lines requiring a gradient
    the other three get none."""
    from directvoxgo_amd.ops import vm_density
    mn, mx, xyz, planes, lines, gout = C.dyadic_case(np.random.default_rng(21))
    t64 = lambda d: {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in d.items()}          # noqa: E731
    rp, rl = t64(planes), t64(lines)
    ref = VO.torch_restatement(rp, rl, torch.from_numpy(xyz).double(), torch.from_numpy(mn).double(),
                               torch.from_numpy(mx).double()).sum(-1)
    ref.backward(torch.from_numpy(gout).double())
    dp = {k: lay_out(p, layout).requires_grad_(wants in ('both', 'planes')) for k, p in planes.items()}
    dl = {k: lay_out(p, layout).requires_grad_(wants in ('both', 'lines')) for k, p in lines.items()}
    out = vm_density(dp, dl if layout == 'cf' else [dl[k] for k in VO.KEYS], cu(xyz), cu(mn), cu(mx))
    assert out.shape == (300,)
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), rtol=1e-5, atol=1e-6)
    out.backward(cu(gout))
    for dev, refs, on in ((dp, rp, wants != 'lines'), (dl, rl, wants != 'planes')):
        for k in VO.KEYS:
            if not on:
                assert dev[k].grad is None
                continue
            assert dev[k].grad.shape == dev[k].shape
            np.testing.assert_allclose(dev[k].grad.cpu().numpy(), refs[k].grad.numpy(), rtol=1e-4, atol=1e-6)


def test_dense_density_at_the_lattice():
    """`dense_density()` of a 6 x 5 x 7 world (one chunk, and two-slab chunks) against the oracle at the lattice of
    `_grid_xyz`, forward bound."""
    from directvoxgo_amd.tensorf import TensoRFVoxGO
    torch.manual_seed(4)
    m = TensoRFVoxGO([-3.25, -2.75, -3.75], [3.25, 2.75, 3.75], num_voxels=268, num_voxels_base=268, alpha_init=1e-2,
                     density_n_comp=3, n_comp=4, rgbnet_width=64).cuda()
    assert [int(v) for v in m.world_size] == [6, 5, 7]
    planes = {k: p.detach().cpu().contiguous().numpy() for k, p in m.density_planes.items()}
    lines = {k: p.detach().cpu().contiguous().numpy() for k, p in m.density_lines.items()}
    xyz = m._grid_xyz((6, 5, 7), 'cpu').reshape(-1, 3).numpy()
    val, A = DO.forward(planes, lines, xyz, m._xyz_min_cpu.numpy(), m._xyz_max_cpu.numpy())
    got = m.dense_density()
    assert tuple(got.shape) == (1, 1, 6, 5, 7) and not got.requires_grad
    err = np.abs(got.reshape(-1).cpu().numpy().astype(np.float64) - val)
    assert (err <= DO.forward_bound(3, A)).all() and np.abs(val).sum() > 0
    assert torch.equal(got, m.dense_density(chunk=2 * 5 * 7)) and torch.equal(got, m.dense_density(chunk=1))
