"""Ray generation and chunked full-image rendering (rows N4 / config 5 of SURVEY.md section 8).

  get_rays / ndc_rays / get_rays_of_a_view   /root/reference/lib/ray_utils.py:9-85 (same argument
                                             meaning; built on the device the pose lives on)
  render_viewpoints                          /root/reference/run.py:57-143: chunks of rays under
                                             no_grad, `render_depth` on (the reference uses 8192; rays
                                             are independent, so the image is identical for any chunk
                                             and 65536 halves the per-view time on MI355X: 43 -> 21 ms
                                             at 800x800); the last chunk may be empty (run.py:91) and
                                             is accepted.  With gt_imgs, PSNR / SSIM per view on the
                                             device (metrics.py), printed as run.py:126-128 does;
                                             savedir writes '{:03d}.png' with Pillow (run.py:132-137).
  evaluate_viewpoints                        the same, returning the per-view metrics as well.
Multi-GPU inference (section 8e): images are embarrassingly parallel -- rank r renders poses
r, r+P, ... and the results are gathered; no all-reduce.
"""
import os

import numpy as np
import torch
import torch.distributed as dist


def get_rays(H, W, K, c2w, inverse_y=False, flip_x=False, flip_y=False, mode='center'):
    dev = c2w.device
    i, j = torch.meshgrid(torch.linspace(0, W - 1, W, device=dev), torch.linspace(0, H - 1, H, device=dev),
                          indexing='ij')
    i, j = i.t().float(), j.t().float()
    if mode == 'center':
        i, j = i + 0.5, j + 0.5
    elif mode == 'random':
        i, j = i + torch.rand_like(i), j + torch.rand_like(j)
    elif mode != 'lefttop':
        raise NotImplementedError
    if flip_x:
        i = i.flip((1,))
    if flip_y:
        j = j.flip((0,))
    fx, fy, cx, cy = float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2])
    if inverse_y:
        dirs = torch.stack([(i - cx) / fx, (j - cy) / fy, torch.ones_like(i)], -1)
    else:
        dirs = torch.stack([(i - cx) / fx, -(j - cy) / fy, -torch.ones_like(i)], -1)
    rays_d = torch.sum(dirs[..., None, :] * c2w[:3, :3], -1)
    rays_o = c2w[:3, 3].expand(rays_d.shape)
    return rays_o, rays_d


def ndc_rays(H, W, focal, near, rays_o, rays_d):
    """lib/ray_utils.py:60-77"""
    t = -(near + rays_o[..., 2]) / rays_d[..., 2]
    rays_o = rays_o + t[..., None] * rays_d
    o0 = -1. / (W / (2. * focal)) * rays_o[..., 0] / rays_o[..., 2]
    o1 = -1. / (H / (2. * focal)) * rays_o[..., 1] / rays_o[..., 2]
    o2 = 1. + 2. * near / rays_o[..., 2]
    d0 = -1. / (W / (2. * focal)) * (rays_d[..., 0] / rays_d[..., 2] - rays_o[..., 0] / rays_o[..., 2])
    d1 = -1. / (H / (2. * focal)) * (rays_d[..., 1] / rays_d[..., 2] - rays_o[..., 1] / rays_o[..., 2])
    d2 = -2. * near / rays_o[..., 2]
    return torch.stack([o0, o1, o2], -1), torch.stack([d0, d1, d2], -1)


def rays_of_view(H, W, K, c2w, ndc, inverse_y, flip_x, flip_y, mode='center', p0=0, n=None, device=None):
    """The rays of pixels [p0, p0 + n) of a view, flat [n, 3], written by ONE kernel (csrc/maintain.hip: rays_of_view) --
    the device form of `get_rays_of_a_view` (lib/ray_utils.py:9-85) for the deterministic pixel modes."""
    import ctypes
    from . import _lib as L
    from ._lib import _flt, _i64, _int, ptr
    assert mode in ('center', 'lefttop')
    dev = torch.device(device) if device is not None else (c2w.device if isinstance(c2w, torch.Tensor) else torch.device('cuda'))
    n = H * W - p0 if n is None else n
    c = np.asarray(c2w.detach().cpu() if isinstance(c2w, torch.Tensor) else c2w, dtype=np.float32)[:3, :4]
    K4 = (ctypes.c_float * 4)(float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2]))
    C12 = (ctypes.c_float * 12)(*[float(v) for v in c.reshape(-1)])
    out = torch.empty((3, max(n, 1), 3), dtype=torch.float32, device=dev)
    with L.device_of(out):
        L.call('dvgo_rays_of_view', _int(H), _int(W), K4, C12, _int(bool(inverse_y)), _int(bool(flip_x)), _int(bool(flip_y)),
               _int(mode == 'center'), _int(bool(ndc)), _flt(float(K[0][0])), _flt(1.0), _i64(p0), _i64(n), ptr(out[0]), ptr(out[1]),
               ptr(out[2]), L.stream_of(out))
    return out[0, :n], out[1, :n], out[2, :n]


def get_rays_of_a_view(H, W, K, c2w, ndc, inverse_y, flip_x, flip_y, mode='center'):
    if isinstance(c2w, torch.Tensor) and c2w.is_cuda and mode in ('center', 'lefttop'):
        o, d, v = rays_of_view(H, W, K, c2w, ndc, inverse_y, flip_x, flip_y, mode)
        return o.view(H, W, 3), d.view(H, W, 3), v.view(H, W, 3)
    rays_o, rays_d = get_rays(H, W, K, c2w, inverse_y=inverse_y, flip_x=flip_x, flip_y=flip_y, mode=mode)
    viewdirs = rays_d / rays_d.norm(dim=-1, keepdim=True)
    if ndc:
        rays_o, rays_d = ndc_rays(H, W, float(K[0][0]), 1., rays_o, rays_d)
    return rays_o, rays_d, viewdirs


def apply_render_factor(HW, Ks, render_factor):
    """run.py:65-69: sizes and intrinsics of copies divided by render_factor (floor division of the float intrinsics too,
    as the reference does)."""
    if render_factor == 0:
        return HW, Ks
    HW = np.copy(HW)
    Ks = np.copy(Ks)
    HW //= render_factor
    Ks[:, :2, :3] //= render_factor
    return HW, Ks


@torch.no_grad()
def render_viewpoints(model, render_poses, HW, Ks, ndc, render_kwargs, flip_x=False, flip_y=False, chunk=65536,
                      distributed=False, ray_kernel=True, gt_imgs=None, savedir=None, render_factor=0, eval_ssim=False,
                      eval_lpips_alex=False, eval_lpips_vgg=False):
    """-> (rgbs [n,H,W,3], depths [n,H,W,1]) as numpy arrays (every rank gets all images when
    ``distributed``).  The metric arguments are those of run.py:57-143; see evaluate_viewpoints."""
    res = evaluate_viewpoints(model, render_poses, HW, Ks, ndc, render_kwargs, flip_x=flip_x, flip_y=flip_y, chunk=chunk,
                              distributed=distributed, ray_kernel=ray_kernel, gt_imgs=gt_imgs, savedir=savedir,
                              render_factor=render_factor, eval_ssim=eval_ssim, eval_lpips_alex=eval_lpips_alex,
                              eval_lpips_vgg=eval_lpips_vgg)
    return res['rgbs'], res['depths']


@torch.no_grad()
def evaluate_viewpoints(model, render_poses, HW, Ks, ndc, render_kwargs, flip_x=False, flip_y=False, chunk=65536,
                        distributed=False, ray_kernel=True, gt_imgs=None, savedir=None, render_factor=0, eval_ssim=False,
                        eval_lpips_alex=False, eval_lpips_vgg=False):
    """Render the views and, given ground truth, score them (run.py:57-143).

    -> {'rgbs': [n,H,W,3], 'depths': [n,H,W,1] (numpy), 'psnr': [n] floats or None, 'ssim': [n] floats or None}.
    Metrics are computed only when ``gt_imgs is not None and render_factor == 0`` (run.py:116), SSIM only with
    ``eval_ssim``; each view is scored on the device from the rendered tensor (gt_imgs[i] may be a numpy array, uploaded,
    or a device tensor).  ``distributed``: every rank scores the views it rendered and the metrics travel with the
    gathered images, so every rank returns the same lists in view order; only rank 0 prints and writes ``savedir``.
    LPIPS is not provided: it needs pretrained AlexNet / VGG weights this project cannot fetch."""
    if eval_lpips_alex or eval_lpips_vgg:
        raise NotImplementedError('LPIPS is not provided: it needs pretrained AlexNet / VGG weights (the lpips package), '
                                  'which this project does not ship or fetch')
    assert len(render_poses) == len(HW) and len(HW) == len(Ks)
    if savedir is not None:
        try:
            import PIL.Image  # noqa: F401
        except ImportError as e:
            raise ImportError('render_viewpoints(savedir=...) writes PNGs with Pillow, which is not installed') from e
    HW, Ks = apply_render_factor(HW, Ks, render_factor)
    score = gt_imgs is not None and render_factor == 0
    if score:
        from .metrics import image_metrics
    world = dist.get_world_size() if distributed else 1
    rank = dist.get_rank() if distributed else 0
    dev = next(model.parameters()).device
    kwargs = dict(render_kwargs, render_depth=True)
    mine = {}
    for i in range(rank, len(render_poses), world):
        H, W = int(HW[i][0]), int(HW[i][1])
        n_pix = H * W
        on_gpu = dev.type == 'cuda' and ray_kernel        # (ray_kernel=False: the torch statement of lib/ray_utils.py, for A/B)
        if not on_gpu:
            c2w = torch.as_tensor(np.asarray(render_poses[i]), dtype=torch.float32, device='cpu' if ray_kernel else dev)
            if not ray_kernel:
                rays_o, rays_d = get_rays(H, W, Ks[i], c2w, inverse_y=kwargs.get('inverse_y', False), flip_x=flip_x, flip_y=flip_y)
                viewdirs = rays_d / rays_d.norm(dim=-1, keepdim=True)
                if ndc:
                    rays_o, rays_d = ndc_rays(H, W, float(Ks[i][0][0]), 1., rays_o, rays_d)
            else:
                rays_o, rays_d, viewdirs = get_rays_of_a_view(H, W, Ks[i], c2w, ndc, inverse_y=kwargs.get('inverse_y', False),
                                                              flip_x=flip_x, flip_y=flip_y)
            rays_o, rays_d, viewdirs = (t.flatten(0, -2).contiguous().to(dev) for t in (rays_o, rays_d, viewdirs))
        out_rgb, out_depth = [], []
        n_chunks = n_pix // chunk + 1                              # run.py:91, last chunk may be empty
        for c in range(n_chunks):
            p0 = chunk * c
            n = max(0, min(chunk, n_pix - p0))
            if on_gpu:       # the chunk's rays straight from the ray-generation kernel: no [H, W, 3] tensors per view
                ro, rd, vd = rays_of_view(H, W, Ks[i], render_poses[i], ndc, kwargs.get('inverse_y', False), flip_x, flip_y,
                                          p0=min(p0, n_pix), n=n, device=dev)
            else:
                ro, rd, vd = rays_o[p0:p0 + n], rays_d[p0:p0 + n], viewdirs[p0:p0 + n]
            res = model(ro, rd, vd, global_step=c, **kwargs)
            out_rgb.append(res['rgb_marched']); out_depth.append(res['depth'])
        rgb = torch.cat(out_rgb).reshape(H, W, 3)
        scores = None
        if score:            # run.py:116-121, on the device before the view leaves it
            gt = gt_imgs[i]
            gt = torch.as_tensor(np.asarray(gt, np.float32) if not isinstance(gt, torch.Tensor) else gt).to(dev, torch.float32)
            s, sse, _ = image_metrics(rgb, gt, max_val=1, filter_size=11 if eval_ssim else 1)
            scores = (sse, s if eval_ssim else None, n_pix * 3)
        mine[i] = (rgb, torch.cat(out_depth).reshape(H, W, 1), scores)

    def host(v):
        rgb, depth, scores = v
        if scores is not None:
            sse, s, n_val = scores
            mse = float(sse[0]) / n_val
            scores = (float('inf') if mse == 0 else float(-10. * np.log10(mse)), float(s[0]) if s is not None else None)
        return rgb.cpu(), depth.cpu(), scores

    mine = {k: host(v) for k, v in mine.items()}
    if distributed and world > 1:
        gathered = [None] * world
        dist.all_gather_object(gathered, mine)
        mine = {k: v for part in gathered for k, v in part.items()}
    idx = sorted(mine)
    rgbs = np.stack([mine[i][0].numpy() for i in idx]) if idx else np.zeros((0,))
    depths = np.stack([mine[i][1].numpy() for i in idx]) if idx else np.zeros((0,))
    psnrs = [mine[i][2][0] for i in idx] if score else None
    ssims = [mine[i][2][1] for i in idx] if score and eval_ssim else None
    if rank == 0:
        if psnrs:
            print('Testing psnr', np.mean(psnrs), '(avg)')
            if eval_ssim:
                print('Testing ssim', np.mean(ssims), '(avg)')
        if savedir is not None:
            from PIL import Image
            from .metrics import to8b
            print(f'Writing images to {savedir}')
            os.makedirs(savedir, exist_ok=True)
            for k in range(len(rgbs)):
                Image.fromarray(to8b(rgbs[k])).save(os.path.join(savedir, '{:03d}.png'.format(k)))
    return {'rgbs': rgbs, 'depths': depths, 'psnr': psnrs, 'ssim': ssims}


# ----------------------------------------------------------------------------------------------
# Training-ray gathering (lib/ray_utils.py:88-183, 283-290)
# ----------------------------------------------------------------------------------------------
@torch.no_grad()
def get_training_rays(rgb_tr, train_poses, HW, Ks, ndc, inverse_y, flip_x, flip_y):
    """Per-image ray tensors [n_img,H,W,3] for same-sized images (lib/ray_utils.py:88-110)."""
    assert len(np.unique(HW, axis=0)) == 1 and len(rgb_tr) == len(train_poses) == len(Ks) == len(HW)
    H, W = int(HW[0][0]), int(HW[0][1])
    dev = rgb_tr.device
    per_view = [get_rays_of_a_view(H, W, Ks[0], torch.as_tensor(np.asarray(c2w), dtype=torch.float32, device=dev),
                                   ndc, inverse_y, flip_x, flip_y) for c2w in train_poses]
    rays_o, rays_d, viewdirs = (torch.stack([v[k] for v in per_view]) for k in range(3))
    return rgb_tr, rays_o, rays_d, viewdirs, [1] * len(rgb_tr)


@torch.no_grad()
def get_training_rays_flatten(rgb_tr_ori, train_poses, HW, Ks, ndc, inverse_y, flip_x, flip_y):
    """All pixels of all (possibly differently sized) images as flat [N,3] tensors (lib/ray_utils.py:113-142)."""
    assert len(rgb_tr_ori) == len(train_poses) == len(Ks) == len(HW)
    dev = rgb_tr_ori[0].device
    rgb, ro, rd, vd, imsz = [], [], [], [], []
    for c2w, img, (H, W), K in zip(train_poses, rgb_tr_ori, HW, Ks):
        assert tuple(img.shape[:2]) == (int(H), int(W))
        o, d, v = get_rays_of_a_view(int(H), int(W), K, torch.as_tensor(np.asarray(c2w), dtype=torch.float32, device=dev),
                                     ndc, inverse_y, flip_x, flip_y)
        rgb.append(img.flatten(0, 1)); ro.append(o.flatten(0, 1)); rd.append(d.flatten(0, 1)); vd.append(v.flatten(0, 1))
        imsz.append(int(H) * int(W))
    return torch.cat(rgb), torch.cat(ro), torch.cat(rd), torch.cat(vd), imsz


@torch.no_grad()
def get_training_rays_in_maskcache_sampling(rgb_tr_ori, train_poses, HW, Ks, ndc, inverse_y, flip_x, flip_y, model,
                                            render_kwargs, rows_per_call=64):
    """Only the rays that hit known-occupied space (lib/ray_utils.py:145-183): `model.hit_coarse_geo`
    (sampler + mask lookup kernels) over 64 image rows at a time."""
    assert len(rgb_tr_ori) == len(train_poses) == len(Ks) == len(HW)
    dev = rgb_tr_ori[0].device
    rgb, ro, rd, vd, imsz = [], [], [], [], []
    n_all = 0
    for c2w, img, (H, W), K in zip(train_poses, rgb_tr_ori, HW, Ks):
        o, d, v = get_rays_of_a_view(int(H), int(W), K, torch.as_tensor(np.asarray(c2w), dtype=torch.float32, device=dev),
                                     ndc, inverse_y, flip_x, flip_y)
        hit = torch.cat([model.hit_coarse_geo(rays_o=o[i:i + rows_per_call], rays_d=d[i:i + rows_per_call], **render_kwargs)
                         for i in range(0, int(H), rows_per_call)])
        rgb.append(img[hit]); ro.append(o[hit]); rd.append(d[hit]); vd.append(v[hit])
        imsz.append(int(hit.sum()))
        n_all += int(H) * int(W)
    return torch.cat(rgb), torch.cat(ro), torch.cat(rd), torch.cat(vd), imsz


def batch_indices_generator(N, BS, seed=None):
    """Endless stream of index batches from a NumPy permutation, reshuffled when exhausted
    (lib/ray_utils.py:283-290)."""
    rng = np.random if seed is None else np.random.RandomState(seed)
    idx, top = torch.from_numpy(rng.permutation(N)), 0
    while True:
        if top + BS > N:
            idx, top = torch.from_numpy(rng.permutation(N)), 0
        yield idx[top:top + BS]
        top += BS
