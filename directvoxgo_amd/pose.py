"""Camera-pose refinement against a DirectVoxGO, a HashVoxGO(raygrad=True), a VMTriPlaneVoxGO(raygrad=True), a
TensoRFVoxGO(raygrad=True) or, for unbounded scenes, a DirectContractedVoxGO(raygrad=True) model (no counterpart in the
reference, whose poses are constants).

Poses from structure-from-motion are off by fractions of a degree, which on a 160^3 - 256^3 grid blurs what the grids could
hold.  This module makes the poses learnable: `CameraRefiner` holds one se(3) correction per view and turns pixels into
rays that are differentiable in it, `DirectVoxGO.forward` renders such rays with gradients flowing back through the sample
positions (ops.ray_points, ops.grid_sample's position gradient: csrc/grid_sample_xyz.hip), and `refine_poses` is the
eager optimisation loop -- poses alone against a trained model (registration of new images included), or poses and model
together.  `refine_poses(..., fused=True)` keeps the render on the fused march (csrc/march_raygrad.hip: march_ray_bwd returns the
ray gradients from the march's own backward) and, with `train_model`, steps the model by a train.TrainStep: the brick
scatter with the Adam update inside it, as in any other training step.  For the contracted model the positions are the
contraction of their rays (ops.contract_points; csrc/contract_raygrad.hip applies the contraction's Jacobian and sums per
ray), on either of its render paths.  For the hash-grid model the colour features' share of the gradient comes from the
hashed gather's own position derivative (ops.hash_sample(position_grad=True); csrc/hash_xyz.hip), on the op-by-op path.
For the two vector-matrix models it comes from the position derivative of planes times lines (ops.vm_sample and, for
TensoRFVoxGO's density, ops.vm_density with position_grad=True; csrc/vm_xyz.hip), on the op-by-op path as well.  Constructed
with raygrad='fused', those three models keep such rays on their fused march: the march's own ray backward
(csrc/march_raygrad.hip) sums, per ray, the density's share of every record and the gradient the samplers returned for the
kept samples' positions.

Pure torch: everything but `refine_poses`' model call runs on CPU tensors too.
"""
import numpy as np
import torch
import torch.nn as nn

_TAYLOR = 1e-4        # |omega| below which the series of the rotation coefficients are used
_TAYLOR_C = 0.25      # ... and of C = (theta - sin theta) / theta^3, whose closed form cancels (see se3_exp)


def _hat(w):
    """[n,3] -> the cross-product matrices [n,3,3]"""
    z = torch.zeros_like(w[:, 0])
    return torch.stack([torch.stack([z, -w[:, 2], w[:, 1]], -1), torch.stack([w[:, 2], z, -w[:, 0]], -1),
                        torch.stack([-w[:, 1], w[:, 0], z], -1)], -2)


def se3_exp(xi):
    """Exponential map of se(3): xi [n,6] = (omega, v) -> [n,3,4] = [R | V v] with, theta = |omega|, K = hat(omega),
        R = I + A K + B K^2,  V = I + B K + C K^2,   A = sin(theta) / theta,  B = (1 - cos(theta)) / theta^2,  C = (theta - sin(theta)) / theta^3
    (Rodrigues).  Below theta = 1e-4 the coefficients are their series in theta^2 (A = 1 - theta^2 / 6, B = 1/2 - theta^2 / 24,
    C = 1/6 - theta^2 / 120), so value and gradient at 0 are finite and exact to first order.  B is evaluated through the half
    angle, and C by its series up to theta^8 below theta = 0.25 (truncation theta^10 / 6.2e9 < 2e-16): theta - sin(theta)
    cancels to theta^3 / 6, which in float32 -- the dtype of CameraRefiner.delta -- leaves no digit at theta = 1e-3 and a
    relative 1e-5 at 0.25."""
    if xi.dim() != 2 or xi.shape[1] != 6:
        raise ValueError('xi must be [n,6]: (omega, v)')
    w, v = xi[:, :3], xi[:, 3:]
    t2 = (w * w).sum(-1)
    small = t2 < _TAYLOR * _TAYLOR
    t2s = torch.where(small, torch.ones_like(t2), t2)          # (keeps the unused branch's gradient finite)
    th = t2s.sqrt()
    half = torch.sin(0.5 * th) / (0.5 * th)
    A = torch.where(small, 1 - t2 / 6, torch.sin(th) / th)
    B = torch.where(small, 0.5 - t2 / 24, 0.5 * half * half)   # (1 - cos) / theta^2 without the cancellation
    small_c = t2 < _TAYLOR_C * _TAYLOR_C
    t2c = torch.where(small_c, torch.ones_like(t2), t2)
    thc = t2c.sqrt()
    series = 1 / 6 - t2 * (1 / 120 - t2 * (1 / 5040 - t2 * (1 / 362880 - t2 / 39916800)))
    C = torch.where(small_c, series, (thc - torch.sin(thc)) / (t2c * thc))
    K = _hat(w)
    K2 = K @ K
    eye = torch.eye(3, dtype=xi.dtype, device=xi.device).expand_as(K)
    R = eye + A[:, None, None] * K + B[:, None, None] * K2
    V = eye + B[:, None, None] * K + C[:, None, None] * K2
    return torch.cat([R, V @ v.unsqueeze(-1)], -1)


class CameraRefiner(nn.Module):
    """Learnable corrections of n camera poses.  One parameter, `delta` [n,6] = (omega, v) per view, zeros at the start.
    The update is LEFT-multiplied, i.e. expressed in the world frame: with exp(delta) = [E | V v] (se3_exp),
        R' = E R,    t' = E t + V v
    for the camera-to-world pose [R | t] given at construction.

    `poses` [n,3,4] (or [n,4,4]) camera-to-world, `HW` [n,2], `Ks` [n,3,3]; inverse_y / flip_x / flip_y as render.get_rays."""

    def __init__(self, poses, HW, Ks, inverse_y=False, flip_x=False, flip_y=False):
        super().__init__()
        as_t = lambda x: x.detach().cpu() if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))     # noqa: E731
        poses = as_t(poses).float()[:, :3, :4].clone()
        n = poses.shape[0]
        HW = as_t(HW).long().reshape(n, 2)
        Ks = as_t(Ks).float().reshape(n, 3, 3)
        self.register_buffer('c2w', poses)
        self.register_buffer('HW', HW)
        self.register_buffer('intr', torch.stack([Ks[:, 0, 0], Ks[:, 1, 1], Ks[:, 0, 2], Ks[:, 1, 2]], -1))   # fx fy cx cy
        self.inverse_y, self.flip_x, self.flip_y = bool(inverse_y), bool(flip_x), bool(flip_y)
        self.delta = nn.Parameter(torch.zeros(n, 6))

    def poses(self):
        """The corrected camera-to-world poses [n,3,4] (differentiable in `delta`)."""
        T = se3_exp(self.delta)
        E = T[:, :, :3]
        return torch.cat([E @ self.c2w[:, :, :3], E @ self.c2w[:, :, 3:] + T[:, :, 3:]], -1)

    def rays(self, view, pix_i, pix_j, ndc=False):
        """Rays of pixels (column pix_i, row pix_j) of views `view` (three [B] integer tensors) -> rays_o, rays_d, viewdirs
        [B,3].  The arithmetic of render.get_rays(mode='center') with its flips and inverse_y, on the corrected poses: equal
        to it at delta = 0, differentiable in `delta`.  viewdirs = rays_d / |rays_d|, detached (the colour heads take no
        gradient for it)."""
        if ndc:
            raise NotImplementedError('CameraRefiner: NDC rays (forward-facing scenes) are not differentiated')
        view = view.long()
        HW = self.HW[view]
        i, j = pix_i.to(self.c2w.dtype), pix_j.to(self.c2w.dtype)
        if self.flip_x:
            i = (HW[:, 1] - 1).to(i.dtype) - i
        if self.flip_y:
            j = (HW[:, 0] - 1).to(j.dtype) - j
        i, j = i + 0.5, j + 0.5
        fx, fy, cx, cy = self.intr[view].unbind(-1)
        if self.inverse_y:
            dirs = torch.stack([(i - cx) / fx, (j - cy) / fy, torch.ones_like(i)], -1)
        else:
            dirs = torch.stack([(i - cx) / fx, -(j - cy) / fy, -torch.ones_like(i)], -1)
        c2w = self.poses()[view]
        rays_d = torch.sum(dirs[..., None, :] * c2w[:, :3, :3], -1)
        rays_o = c2w[:, :3, 3]
        viewdirs = (rays_d / rays_d.norm(dim=-1, keepdim=True)).detach()
        return rays_o.contiguous(), rays_d.contiguous(), viewdirs.contiguous()


def _contracted(model):
    from .dcvgo import DirectContractedVoxGO
    return type(model) is DirectContractedVoxGO


def _hashed(model):
    from .hashgrid import HashVoxGO
    return type(model) is HashVoxGO


def _vm(model):
    from .tensorf import TensoRFVoxGO
    from .vm import VMTriPlaneVoxGO
    return type(model) in (VMTriPlaneVoxGO, TensoRFVoxGO)


def _takes_raygrad(model):
    """The classes that differentiate their rays only when constructed with raygrad=True."""
    return _contracted(model) or _hashed(model) or _vm(model)


def _supported(model):
    from .dvgo import DirectVoxGO
    if _takes_raygrad(model):
        return model.raygrad
    return type(model) is DirectVoxGO and model.posbase_pe == 0


def refine_poses(model, refiner, images, cfg_train, render_kwargs, n_iters, n_rand, lrate_pose, train_model=False, seed=None,
                 fused=False):
    """Optimise `refiner.delta` against `images` by rendering `model` from the corrected poses -> the loss of every
    iteration (floats).

    An eager loop: `n_rand` random pixels over all views (None, or at least as many as there are pixels: every pixel, every
    iteration), `refiner.rays`, `model(...)`, train.render_loss, backward, torch.optim.Adam(lr=lrate_pose) on `delta`.
    `images`: [n,H,W,3] or a list of [H_v,W_v,3], float, on the model's device.  With `train_model` the model's parameters
    are stepped in the same iteration by a second optimiser (train.create_optimizer_or_freeze_model(model, cfg_train, 0));
    without it they receive no gradient and `.grad` is left alone.

    `fused=True` (a model with `model.fused`, else ValueError): `DirectVoxGO.fused_raygrad` is set on the model for the
    duration of the loop, so the render is the fused march and `delta`'s gradient comes from dvgo_march_ray_bwd; with
    `train_model` the model is then stepped by a `train.TrainStep(model, cfg_train, render_kwargs)` -- per iteration
    `opt_pose.zero_grad()`, `loss = step(rays_o, rays_d, viewdirs, target, it + 1)`, `opt_pose.step()` -- whose backward
    updates both grids inside the brick scatter where the optimizer allows it (their `.grad` stays None).

    A `DirectContractedVoxGO(raygrad=True)` (unbounded scenes) renders by its own path, fused march or op by op as it was
    constructed, with the rays differentiated through the contraction (csrc/contract_raygrad.hip;
    DirectContractedVoxGO._render states the stop-gradients).  `fused=True` then requires `model.fused_march`
    (ValueError otherwise) and, with `train_model`, steps the model by a `train.TrainStep`, whose plan for this model is dense
    gradients and the optimizer's own step; `cfg_train['weight_distortion']` adds the distortion loss as in training.

    A `HashVoxGO(raygrad=True)` renders such rays op by op (DirectVoxGO._forward_raygrad; the features' position derivative
    is csrc/hash_xyz.hip) whatever `model.fused` says: `fused=True` is a ValueError for it, and `train_model` steps density,
    table and head by the eager optimiser.  A `HashVoxGO(raygrad='fused')` (the instance carries `fused_raygrad`) is accepted
    with `fused=True`: the render is `fused_march(positions=True, raygrad=True)`, `delta`'s gradient comes from
    dvgo_march_ray_bwd_pts (csrc/march_raygrad.hip), and with `train_model` the model is stepped by a `train.TrainStep`.

    A `VMTriPlaneVoxGO(raygrad=True)` and a `TensoRFVoxGO(raygrad=True)` render such rays op by op as well
    (DirectVoxGO._forward_raygrad; the position derivative of planes times lines is csrc/vm_xyz.hip, for the features and,
    in TensoRFVoxGO, for the density) whatever `model.fused` and `model.fused_march` say: `fused=True` is a ValueError for
    them, and `train_model` steps planes, lines, basis, the density tensors and the head by the eager optimiser.
    Constructed with `raygrad='fused'` they are accepted with `fused=True` as the hash-grid model is: the VMTriPlaneVoxGO on
    `fused_march(positions=True, raygrad=True)`, the TensoRFVoxGO on `fused_march_vm(raygrad=True)` (dvgo_march_vm_ray_bwd),
    which requires `model.fused_march` (ValueError naming `fused_march` otherwise); with `train_model` a `train.TrainStep`
    steps the model.  The instance's `fused_raygrad` is left as it was found.

    The gradient reaches `delta` through the sample positions only (DirectVoxGO._forward_raygrad states the stop-gradients).
    Supported: a plain DirectVoxGO with posbase_pe == 0, a HashVoxGO, a VMTriPlaneVoxGO or a TensoRFVoxGO constructed with
    raygrad=True (with fused=False only) or raygrad='fused' (either) and a DirectContractedVoxGO constructed with raygrad=True.
    NDC rays, posbase_pe heads, data-parallel steps and the plain tri-plane / LIIF / bilinear-decoder models stay refused.  DirectMPIGO (NDC warp),
    the tri-plane, LIIF and bilinear-decoder models (plane samplers) and positional-encoding heads (position input of the
    head) lack their derivative and raise NotImplementedError, as do a DirectContractedVoxGO, a HashVoxGO, a VMTriPlaneVoxGO
    and a TensoRFVoxGO without raygrad."""
    if not _supported(model):
        kind = type(model).__name__ + (' with posbase_pe > 0' if getattr(model, 'posbase_pe', 0) > 0 else '')
        hint = ': construct it with raygrad=True' if _takes_raygrad(model) else ''
        raise NotImplementedError(f'refine_poses: {kind} is not supported: only a plain DirectVoxGO with posbase_pe == 0 has '
                                  f'the position derivative of its sampler{hint}')
    contracted = _contracted(model)
    on_march = bool(model.__dict__.get('fused_raygrad'))           # raygrad='fused': the instance's own attribute
    if fused and _hashed(model) and not on_march:
        raise ValueError('refine_poses(fused=True): HashVoxGO differentiates its rays on the op-by-op path only '
                         '(fused_march(positions=True) has no ray gradient by default): call it with fused=False, or construct it with '
                         "raygrad='fused'")
    if fused and _vm(model) and not on_march:
        raise ValueError(f'refine_poses(fused=True): {type(model).__name__} differentiates its rays on the op-by-op path only '
                         '(the fused marches over positions and over the decomposed density have no ray gradient by default): call it '
                         "with fused=False, or construct it with raygrad='fused'")
    if fused and _vm(model) and hasattr(model, 'fused_march') and not model.fused_march:
        raise ValueError(f'refine_poses(fused=True) needs a {type(model).__name__} on the fused march (fused_march=True)')
    if fused and contracted and not model.fused_march:
        raise ValueError('refine_poses(fused=True) needs a DirectContractedVoxGO on the fused march (fused_march=True)')
    if fused and not getattr(model, 'fused', False):
        raise ValueError('refine_poses(fused=True) needs a model on the fused march (model.fused)')
    from .train import TrainStep, create_optimizer_or_freeze_model, render_loss
    dev = refiner.delta.device
    HW = refiner.HW
    n = HW.shape[0]
    if isinstance(images, torch.Tensor):
        images = list(images)
    assert len(images) == n, 'one image per view'
    flat = torch.cat([im.reshape(-1, 3) for im in images]).to(dev).float()
    npix = HW[:, 0] * HW[:, 1]
    base = torch.cumsum(npix, 0) - npix
    total = int(npix.sum())
    every = n_rand is None or n_rand >= total
    if every:
        view = torch.repeat_interleave(torch.arange(n, device=dev), npix)
        p = torch.arange(total, device=dev) - base[view]
        pix_j, pix_i = p // HW[view, 1], p % HW[view, 1]
    gen = torch.Generator(device='cpu')
    if seed is not None:
        gen.manual_seed(int(seed))
    opt_pose = torch.optim.Adam([refiner.delta], lr=lrate_pose)
    step = TrainStep(model, cfg_train, render_kwargs) if (fused and train_model) else None
    opt_model = create_optimizer_or_freeze_model(model, cfg_train, 0) if (train_model and step is None) else None
    losses = []
    was = model.__dict__.get('fused_raygrad')          # (the class attribute unless somebody set it on the instance)
    fused_flag = fused and not contracted              # (the contracted model's render path is its own: fused_march)
    if fused_flag:
        model.fused_raygrad = True
    try:
        for it in range(int(n_iters)):
            if not every:
                view = torch.randint(n, (n_rand,), generator=gen).to(dev)
                u = torch.rand((2, n_rand), generator=gen).to(dev)
                pix_i = (u[0] * HW[view, 1]).long().minimum(HW[view, 1] - 1)
                pix_j = (u[1] * HW[view, 0]).long().minimum(HW[view, 0] - 1)
            target = flat[base[view] + pix_j * HW[view, 1] + pix_i]
            rays_o, rays_d, viewdirs = refiner.rays(view, pix_i, pix_j)
            if step is not None:
                opt_pose.zero_grad(set_to_none=True)
                loss = step(rays_o, rays_d, viewdirs, target, it + 1)
                opt_pose.step()
                losses.append(loss)
                continue
            res = model(rays_o, rays_d, viewdirs, global_step=None, **render_kwargs)
            loss = render_loss(res, target, rays_o.shape[0], cfg_train)
            opt_pose.zero_grad(set_to_none=True)
            if opt_model is not None:
                opt_model.zero_grad(set_to_none=True)
                loss.backward()
                opt_model.step()
            else:
                loss.backward(inputs=[refiner.delta])
            opt_pose.step()
            losses.append(loss.detach())
    finally:
        if fused_flag:
            if was is None:
                del model.fused_raygrad
            else:
                model.fused_raygrad = was
    return [float(x) for x in losses]          # (read back once, after the loop)
