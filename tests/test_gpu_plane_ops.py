"""GPU: what the four plane ops share on the host (ops._kernel_tensors, ops._scatter_grads): the relayout rule, the layout
of the gradients they return and the masking by need, for triplane_sample, vm_sample, liif_gather and plane_rows on
channel-first, channels-last and mixed planes, below and above the size at which the ops hand the kernels channels-last
copies (the samples outnumber the largest plane's 42 texels).

The forward does not depend on the layout, so it equals the raw entry point on channels-last copies bit for bit.  The
gradients come out of float atomics, whose order differs between layouts: each is held to the bound of its op's own kernel
test against the float64 oracle, (n + 2) U A per texel with n contributions (test_gpu_triplane, test_gpu_liif,
test_gpu_interp) and (n + 12) U A for the product of plane and line (test_gpu_vm); a texel nothing reaches is exactly 0.
"""
import functools

import numpy as np
import pytest
import torch

import interp_oracle as IO
import liif_oracle as LO
import triplane_oracle as TO
import vm_oracle as VO
from test_gpu_triplane import MN, MX, cu, points

pytestmark = pytest.mark.gpu

OPS = ('triplane_sample', 'vm_sample', 'liif_gather', 'plane_rows')
SIZES = {'xy': (6, 7), 'yz': (3, 9), 'zx': (8, 2)}
LINES = {'xy': 5, 'yz': 1, 'zx': 9}
C, WS, NF = 4, (5, 6, 7), 2
TEXELS = max(h * w for h, w in SIZES.values())
LAYOUTS = {'cf': ('cf', 'cf', 'cf'), 'cl': ('cl', 'cl', 'cl'), 'mixed': ('cf', 'cl', 'cl')}
EXTRA = {'triplane_sample': 2, 'vm_sample': 12, 'liif_gather': 2, 'plane_rows': 2}      # the ops' own kernel tests' bounds


@functools.lru_cache(maxsize=None)
def case(op, M):
    """planes (and lines), positions, the gradient handed to backward and the oracle's (gradient, A, n) per tensor"""
    rng = np.random.default_rng(7 + M)
    planes = {k: rng.standard_normal((1, C, *hw)).astype(np.float32) for k, hw in SIZES.items()}
    lines = {k: rng.standard_normal((1, C, n, 1)).astype(np.float32) for k, n in LINES.items()}
    xyz = points(M, SIZES, rng)
    shapes = {k: p.shape[1:] for k, p in planes.items()}
    tensors = [planes[k] for k in TO.KEYS]
    if op == 'triplane_sample':
        gout = rng.standard_normal((M, 3 * C)).astype(np.float32)
        ref = TO.backward(shapes, xyz, MN, MX, gout, 'concat')
    elif op == 'vm_sample':
        gout = rng.standard_normal((M, 3 * C)).astype(np.float32)
        rp, rl = VO.backward(planes, lines, xyz, MN, MX, gout)
        tensors += [lines[k] for k in TO.KEYS]
        return tensors, xyz, gout, [rp[k] for k in TO.KEYS] + [rl[k] for k in TO.KEYS]
    elif op == 'liif_gather':
        gout = rng.standard_normal((3, 4, M, C + 4)).astype(np.float32)
        ref = LO.scatter(shapes, xyz, MN, MX, WS, gout, True)
    else:
        gout = rng.standard_normal((3, M, IO.columns(C, NF, True)[1])).astype(np.float32)
        ref = IO.scatter(shapes, xyz, MN, MX, gout)
    return tensors, xyz, gout, [ref[k] for k in TO.KEYS]


def lay(p, layout):
    t = cu(p)
    return t if layout == 'cf' else t.contiguous(memory_format=torch.channels_last)


def sample(op, t, xyz, mn, mx, raw=False):
    """-> every output of the op (raw: of the entry point under it, on the strides given); the first carries the gradient"""
    from directvoxgo_amd import ops
    if op == 'triplane_sample':
        return ((ops.triplane_fwd if raw else ops.triplane_sample)(t, xyz, mn, mx, 'concat'),)
    if op == 'vm_sample':
        return ((ops.vm_fwd if raw else ops.vm_sample)(t[:3], t[3:], xyz, mn, mx),)
    if op == 'liif_gather':
        return tuple((ops.liif_gather_fwd if raw else ops.liif_gather)(t, xyz, mn, mx, WS, True, True))
    return ((ops.plane_rows_fwd if raw else ops.plane_rows)(t, xyz, mn, mx, WS, NF, True),)


def check_gradient(op, grad, ref):
    g, A, n = ref
    gg = grad[0].cpu().numpy().astype(np.float64).reshape(g.shape)           # (a line's [R,N,1] -> [R,N])
    err, bound = np.abs(gg - g), (n[None] + EXTRA[op]) * TO.U * A
    print(f'{op}: worst gradient err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}')
    assert (err <= bound).all(), float((err - bound).max())
    assert (gg[:, n == 0] == 0).all()


def run(op, M, layout, relayout, frozen=()):
    arrays, xyz, gout, ref = case(op, M)
    los = LAYOUTS[layout] * (len(arrays) // 3)
    tensors = [lay(p, lo).requires_grad_(i not in frozen) for i, (p, lo) in enumerate(zip(arrays, los))]
    dx, mn, mx = cu(xyz), cu(MN), cu(MX)
    outs = sample(op, tensors, dx, mn, mx)
    with torch.no_grad():
        same = sample(op, [t.detach().contiguous(memory_format=torch.channels_last) for t in tensors], dx, mn, mx, raw=True)
    assert len(outs) == len(same) and all(torch.equal(a, b) for a, b in zip(outs, same))
    live = [i for i in range(len(tensors)) if i not in frozen]
    grads = dict(zip(live, torch.autograd.grad(outs[0], [tensors[i] for i in live], cu(gout))))
    for i, t in enumerate(tensors):
        if i in frozen:
            continue
        copied = relayout and not (t.stride(1) == 1 or t.shape[1] == 1)
        want = torch.empty_like(t, memory_format=torch.channels_last if copied else torch.preserve_format).stride()
        assert grads[i].shape == t.shape and grads[i].stride() == want, (i, grads[i].stride(), want)
        check_gradient(op, grads[i], ref[i])
    return tensors, outs


@pytest.mark.parametrize('layout', list(LAYOUTS))
@pytest.mark.parametrize('M', [8, 64])
@pytest.mark.parametrize('op', OPS)
def test_forward_bits_and_gradient_layout(op, M, layout):
    """M = 8 < 42 texels: the kernels run on the strides given and every gradient has its parameter's; M = 64: whatever is
    not channels-last reaches the kernels as a copy and its gradient comes back channels-last."""
    assert (M >= TEXELS) == (M == 64)
    run(op, M, layout, relayout=M >= TEXELS)


@pytest.mark.parametrize('op', OPS)
def test_a_plane_that_wants_no_gradient_gets_none(op):
    arrays, xyz, gout, ref = case(op, 64)
    tensors, outs = run(op, 64, 'cf', relayout=True, frozen=(1,))             # (the others' gradients: checked in there)
    for t in tensors:
        t.grad = None
    outs = sample(op, tensors, cu(xyz), cu(MN), cu(MX))
    outs[0].backward(cu(gout))
    assert tensors[1].grad is None
    for i, t in enumerate(tensors):
        if i != 1:
            assert t.grad is not None and t.grad.shape == t.shape
            check_gradient(op, t.grad, ref[i])


@pytest.mark.parametrize('op', OPS)
def test_relayout_switched_off_takes_the_strided_branch(op, monkeypatch):
    from directvoxgo_amd import ops
    monkeypatch.setattr(ops, 'TRIPLANE_RELAYOUT', False)
    run(op, 64, 'mixed', relayout=False)
