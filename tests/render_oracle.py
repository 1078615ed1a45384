"""CPU statement of a whole render + backward on the oracle's functions, test infrastructure.

Built only from what oracle/oracle.py exports (the scalar C ops, in the reference's op order) and plain torch on the CPU
for the colour head and the loss, so that it runs at the product's real sizes (160^3 x 12 with 2 M samples, 256^3,
343 x 382 x 128) in seconds.  It is pinned against the reference's own orchestration by tests/test_render_oracle_host.py
(the golden forward fixtures) before any GPU test trusts it.

  Scene(...)                        grids, mask, bbox and head of one model (host copies; `k0` may be a strided view)
  forward(scene, rays, ...)         lib/dvgo.py:450-577 / lib/dmpigo.py:200-283 -> the reference's dict, plus
                                    `step_id`, `feat` (per-sample features), `pts` and the state `backward` needs
  backward(scene, out, g_*)         upstream gradients of rgb_marched / alphainv_last / raw_rgb / weights ->
                                    grad_density, grad_k0 (channels-first [C,X,Y,Z]), grad_rgbnet_<name>
  loss_and_grads(scene, out, ...)   the run.py loss (run.py:377-386) by autograd on the outputs, then `backward`
  hit_coarse_geo(scene, rays, ...)  lib/dvgo.py:412-423

The colour head takes a `dtype`: float32 reproduces the fixtures, float64 is the arbiter at full size.  Every other
step is the oracle's float32.
"""
import numpy as np
import torch

from oracle import oracle as O

f32 = np.float32
HEAD_CHUNK = 1 << 18            # rows of the colour head per autograd pass (bounds host memory at 2 M samples)


class Scene:
    """density [X,Y,Z] or [1,1,X,Y,Z]; k0 [C,X,Y,Z] or [1,C,X,Y,Z] (any strides: a channels-last view is read in
    place); mask [X,Y,Z] bool; rgbnet: {state-dict key: array} of the nn.Sequential head, or None (sigmoid(k0));
    mpi_depth > 0 selects DirectMPIGO (NDC sampler, act_shift 0, voxel_size_ratio = 256 / mpi_depth)."""

    def __init__(self, xyz_min, xyz_max, density, k0, mask, fast_color_thres, act_shift=0.0, voxel_size=None,
                 voxel_size_ratio=1.0, rgbnet=None, direct=True, viewbase_pe=4, mpi_depth=0):
        self.xyz_min = np.asarray(xyz_min, f32).reshape(3)
        self.xyz_max = np.asarray(xyz_max, f32).reshape(3)
        density = np.asarray(density, f32)
        self.density = np.ascontiguousarray(density.reshape(density.shape[-3:]))[None]
        k0 = np.asarray(k0)
        self.k0 = k0[0] if k0.ndim == 5 else k0
        assert self.k0.dtype == np.float32 and self.k0.shape[1:] == self.density.shape[1:]
        self.mask = np.ascontiguousarray(np.asarray(mask, bool))
        self.thres = f32(fast_color_thres)
        self.act_shift = float(act_shift)
        self.voxel_size = None if voxel_size is None else f32(voxel_size)
        self.voxel_size_ratio = f32(voxel_size_ratio)
        self.mpi_depth = int(mpi_depth)
        self.direct, self.viewbase_pe = bool(direct), int(viewbase_pe)
        self.head = None
        if rgbnet is not None:
            keys = sorted((k for k in rgbnet if k.endswith('.weight')), key=lambda k: [int(p) for p in k.split('.')[:-1]])
            self.head = [(k[:-len('weight')], np.asarray(rgbnet[k], f32), np.asarray(rgbnet[k[:-len('weight')] + 'bias'], f32))
                         for k in keys]
        # MaskCache (lib/dvgo.py:600-602), float32 tensor maths as the reference writes it
        mn, mx = torch.from_numpy(self.xyz_min), torch.from_numpy(self.xyz_max)
        scale = (torch.tensor(list(self.mask.shape), dtype=torch.float32) - 1) / (mx - mn)
        self.mask_scale, self.mask_shift = scale.numpy(), (-mn * scale).numpy()

    @property
    def world_size(self):
        return self.density.shape[1:]


def _sample(scene, rays_o, rays_d, near, far, stepsize):
    """sample_ray (lib/dvgo.py:425-448 / lib/dmpigo.py:173-198): in-box points, ray_id, step_id."""
    if scene.mpi_depth:
        n_samples = int((scene.mpi_depth - 1) / stepsize) + 1
        pts, out = O.sample_ndc_pts_on_rays(rays_o, rays_d, scene.xyz_min, scene.xyz_max, n_samples)
        keep = ~out
        N = rays_o.shape[0]
        ray_id = np.broadcast_to(np.arange(N, dtype=np.int64)[:, None], keep.shape)[keep]
        step_id = np.broadcast_to(np.arange(n_samples, dtype=np.int64)[None, :], keep.shape)[keep]
        return pts[keep], ray_id, step_id
    stepdist = f32(f32(stepsize) * scene.voxel_size)
    pts, out, ray_id, step_id = O.sample_pts_on_rays(rays_o, rays_d, scene.xyz_min, scene.xyz_max, near, far,
                                                     float(stepdist))[:4]
    keep = ~out
    return pts[keep], ray_id[keep], step_id[keep]


def _interval(scene, stepsize):
    return float(f32(f32(stepsize) * scene.voxel_size_ratio))


def hit_coarse_geo(scene, rays_o, rays_d, near, far, stepsize):
    """lib/dvgo.py:412-423: a ray hits when any of its in-box samples lies in known-occupied space."""
    pts, ray_id, _ = _sample(scene, np.asarray(rays_o, f32), np.asarray(rays_d, f32), near, far, stepsize)
    hit = np.zeros(len(rays_o), bool)
    hit[ray_id[O.maskcache_lookup(scene.mask, pts, scene.mask_scale, scene.mask_shift)]] = True
    return hit


def viewdir_embedding(viewdirs, pe, dtype):
    """lib/dvgo.py:532-534: [d, sin(d * 2^i), cos(d * 2^i)] with the frequencies fastest within each axis."""
    vd = torch.as_tensor(np.asarray(viewdirs, f32)).to(dtype)
    freq = torch.tensor([2.0 ** i for i in range(pe)], dtype=torch.float32).to(dtype)
    emb = (vd.unsqueeze(-1) * freq).flatten(-2)
    return torch.cat([vd, emb.sin(), emb.cos()], -1)


def _head(scene, params, feat, emb):
    """rgbnet + sigmoid on one chunk of rows (lib/dvgo.py:512-541, lib/dmpigo.py:246-257)."""
    if scene.head is None:
        return torch.sigmoid(feat)
    x = torch.cat([feat if scene.direct else feat[:, 3:], emb], -1)
    for i, (W, b) in enumerate(params):
        x = torch.addmm(b, x, W.t())
        if i + 1 < len(params):
            x = torch.relu(x)
    return torch.sigmoid(x if scene.direct else x + feat[:, :3])


def _head_params(scene, dtype, requires_grad=False):
    return [(torch.from_numpy(W).to(dtype).requires_grad_(requires_grad),
             torch.from_numpy(b).to(dtype).requires_grad_(requires_grad)) for _, W, b in (scene.head or [])]


def forward(scene, rays_o, rays_d, viewdirs, near, far, stepsize, bg, dtype=torch.float32, render_depth=True):
    """The reference's forward in its op order on the oracle.  Returns numpy arrays: alphainv_last [N], weights [M],
    rgb_marched [N,3], raw_alpha [M], raw_rgb [M,3] (in `dtype`), ray_id [M], step_id [M], feat [M,C], pts [M,3],
    depth [N]; and under '_state' what `backward` needs."""
    rays_o, rays_d = np.asarray(rays_o, f32), np.asarray(rays_d, f32)
    N = rays_o.shape[0]
    interval = _interval(scene, stepsize)
    # 1. sample, 2. skip known free space
    pts, ray_id, step_id = _sample(scene, rays_o, rays_d, near, far, stepsize)
    sel = O.maskcache_lookup(scene.mask, pts, scene.mask_scale, scene.mask_shift)
    pts, ray_id, step_id = pts[sel], ray_id[sel], step_id[sel]
    # 3. density, 4. activation + alpha filter
    density = O.grid_sample_fwd(scene.density, pts, scene.xyz_min, scene.xyz_max, use_fma=True)[:, 0]
    exp_d, alpha = O.raw2alpha(density, scene.act_shift, interval)
    if scene.thres > 0:
        sel = alpha > scene.thres
        pts, ray_id, step_id, exp_d, alpha = pts[sel], ray_id[sel], step_id[sel], exp_d[sel], alpha[sel]
    # 5. transmittance + weight filter
    w_all, T, last, i_start, i_end = O.alpha2weight(alpha, ray_id, N)
    keep = w_all > scene.thres if scene.thres > 0 else np.ones(w_all.shape, bool)
    state = dict(pts1=pts, exp_d=exp_d, alpha1=alpha, ray_id1=ray_id, w_all=w_all, T=T, i_start=i_start, i_end=i_end,
                 keep=keep, interval=interval, bg=float(bg), dtype=dtype, N=N)
    weights, alpha_k, pts, ray_id, step_id = w_all[keep], alpha[keep], pts[keep], ray_id[keep], step_id[keep]
    # 6. features from the grid as it is stored
    feat = O.grid_sample_fwd(scene.k0, pts, scene.xyz_min, scene.xyz_max, use_fma=True)
    # 7. colour head (torch, `dtype`)
    emb = viewdir_embedding(viewdirs, scene.viewbase_pe, dtype) if scene.head is not None else None
    params = _head_params(scene, dtype)
    rgb = np.empty((feat.shape[0], 3), np.float64 if dtype == torch.float64 else f32)
    with torch.no_grad():
        for s in range(0, feat.shape[0], HEAD_CHUNK):
            sl = slice(s, s + HEAD_CHUNK)
            e = emb[torch.from_numpy(ray_id[sl])] if emb is not None else None
            rgb[sl] = _head(scene, params, torch.from_numpy(feat[sl]).to(dtype), e).numpy()
    # 8. per-ray sums (float32: the oracle's segment sum; float64: the same sum in double)
    if dtype == torch.float64:
        rgb_marched = np.zeros((N, 3))
        np.add.at(rgb_marched, ray_id, weights[:, None].astype(np.float64) * rgb)
        rgb_marched += last[:, None].astype(np.float64) * bg
    else:
        rgb_marched = O.segment_sum(weights[:, None] * rgb, ray_id, N) + last[:, None] * f32(bg)
    out = dict(alphainv_last=last, weights=weights, rgb_marched=rgb_marched, raw_alpha=alpha_k, raw_rgb=rgb,
               ray_id=ray_id, step_id=step_id, feat=feat, pts=pts, _state=state, _emb=emb)
    # 9. depth
    if render_depth:
        out['depth'] = O.segment_sum(weights * step_id.astype(f32), ray_id, N)
    return out


def backward(scene, out, g_rgb_marched, g_alphainv_last, g_raw_rgb=None, g_weights=None):
    """Chain the upstream gradients of the forward's outputs through the composite, the colour head (torch autograd,
    in the forward's dtype) and the oracle's alpha2weight_backward(fma) / raw2alpha_backward / grid_sample_bwd.
    Returns grad_density [X,Y,Z], grad_k0 [C,X,Y,Z] (channels-first, float32) and grad_rgbnet_<key>."""
    st = out['_state']
    dtype, N = st['dtype'], st['N']
    npd = np.float64 if dtype == torch.float64 else f32
    ray_id, w, rgb = out['ray_id'], out['weights'].astype(npd), out['raw_rgb'].astype(npd)
    gm = np.asarray(g_rgb_marched, npd)[ray_id]
    # composite: rgb_marched = sum_ray w * rgb + alphainv_last * bg
    g_w = (gm * rgb).sum(-1)
    if g_weights is not None:
        g_w = g_w + np.asarray(g_weights, npd)
    g_rgb = w[:, None] * gm
    if g_raw_rgb is not None:
        g_rgb = g_rgb + np.asarray(g_raw_rgb, npd)
    g_last = np.asarray(g_alphainv_last, npd) + st['bg'] * np.asarray(g_rgb_marched, npd).sum(-1)
    # colour head, chunk by chunk (weight gradients summed over the chunks in `dtype`)
    params = _head_params(scene, dtype, requires_grad=True)
    flat = [p for pair in params for p in pair]
    acc = [torch.zeros_like(p) for p in flat]
    feat = out['feat']
    g_feat = np.empty(feat.shape, f32)
    emb = out['_emb']
    for s in range(0, feat.shape[0], HEAD_CHUNK):
        sl = slice(s, s + HEAD_CHUNK)
        x = torch.from_numpy(feat[sl]).to(dtype).requires_grad_(True)
        e = emb[torch.from_numpy(ray_id[sl])] if emb is not None else None
        y = _head(scene, params, x, e)
        grads = torch.autograd.grad(y, [x] + flat, torch.from_numpy(g_rgb[sl]), allow_unused=True)
        g_feat[sl] = grads[0].numpy()
        for a, g in zip(acc, grads[1:]):
            a += g
    res = {'g_feat': g_feat}
    for (name, _, _), gw, gb in zip(scene.head or [], acc[0::2], acc[1::2]):
        res['grad_rgbnet_' + name + 'weight'] = gw.numpy()
        res['grad_rgbnet_' + name + 'bias'] = gb.numpy()
    # transmittance: gradients of the weights the filter dropped are zero
    g_w_all = np.zeros(st['w_all'].shape, f32)
    g_w_all[st['keep']] = g_w
    g_alpha = O.alpha2weight_backward(st['alpha1'], st['w_all'], st['T'], out['alphainv_last'], st['i_start'],
                                      st['i_end'], N, g_w_all, g_last.astype(f32), fma=True)
    g_dens = O.raw2alpha_backward(st['exp_d'], g_alpha, st['interval'])
    X, Y, Z = scene.world_size
    res['grad_density'] = O.grid_sample_bwd(g_dens[:, None], (1, X, Y, Z), st['pts1'], scene.xyz_min, scene.xyz_max)[0]
    res['grad_k0'] = O.grid_sample_bwd(g_feat, (feat.shape[1], X, Y, Z), out['pts'], scene.xyz_min, scene.xyz_max)
    return res


def relu_margin(scene, out):
    """Per sample: the smallest |pre-activation| of a hidden ReLU unit relative to the sum of the magnitudes of its terms,
    in float64.  A float32 head (any summation order) can give a unit whose margin is below its dot product's rounding
    bound (~1e-5 for 128 terms) the other sign: that sample's feature gradient is then legitimately another one."""
    feat, emb, ray_id = out['feat'], out['_emb'], out['ray_id']
    params = _head_params(scene, torch.float64)
    margin = np.full(feat.shape[0], np.inf)
    with torch.no_grad():
        for s in range(0, feat.shape[0], HEAD_CHUNK):
            sl = slice(s, s + HEAD_CHUNK)
            x = torch.from_numpy(feat[sl]).double()
            x = torch.cat([x if scene.direct else x[:, 3:], emb[torch.from_numpy(ray_id[sl])].double()], -1)
            m = torch.full((x.shape[0],), float('inf'), dtype=torch.float64)
            for W, b in params[:-1]:
                h = torch.addmm(b, x, W.t())
                mag = torch.addmm(b.abs(), x.abs(), W.abs().t())
                m = torch.minimum(m, (h.abs() / mag.clamp_min(1e-300)).amin(1))
                x = torch.relu(h)
            margin[sl] = m.numpy()
    return margin


def loss_and_grads(scene, out, target, w_main=1.0, w_ent=0.001, w_per=0.01):
    """run.py:377-386 (tests/test_gpu_forward.py::loss_fn) by autograd on the outputs, in the head's dtype, then
    `backward`.  Returns (loss, gradients)."""
    dtype = out['_state']['dtype']
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    marched = t(out['rgb_marched']).requires_grad_(True)
    last = t(out['alphainv_last']).requires_grad_(True)
    raw = t(out['raw_rgb']).requires_grad_(True)
    tgt = t(target)
    loss = w_main * torch.nn.functional.mse_loss(marched, tgt)
    pout = last.clamp(1e-6, 1 - 1e-6)
    loss = loss + w_ent * (-(pout * torch.log(pout) + (1 - pout) * torch.log(1 - pout)).mean())
    rgbper = (raw - tgt[torch.from_numpy(out['ray_id'])]).pow(2).sum(-1)
    loss = loss + w_per * ((rgbper * t(out['weights'])).sum() / tgt.shape[0])
    gm, gl, gr = torch.autograd.grad(loss, [marched, last, raw])
    return float(loss.detach()), backward(scene, out, gm.numpy(), gl.numpy(), gr.numpy())
