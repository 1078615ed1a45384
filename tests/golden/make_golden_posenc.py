"""Generate the fixtures of the positional-encoding colour head (posbase_pe > 0, lib/dvgo.py:97-107,528-534) by RUNNING THE
REFERENCE's own Python, through make_golden.import_reference() (a scratch copy with the oracle-backed natives), never in
place.  Runs only where the reference tree exists; the files it writes are committed:

  forward_fine_posenc.npz      posbase_pe = 10, width 128, rgbnet_direct=True: the head configs/nerf/lego.py gets when its
                               `posbase_pe=10` line is switched on.  make_golden.gen_forward's scene, rays and keys
                               (+ `posbase_pe`, and `head_input`: the [M, d_in] rows the reference fed its colour
                               head, positions first), without grad_k0: the reference leaves k0.grad None.
  forward_fine_posenc_p4.npz   posbase_pe = 4, rgbnet_direct=False: pins that there is no diffuse term.
  ref_checkpoint_posenc.tar    a small checkpoint written as run.py writes it (make_golden.gen_checkpoint's recipe) by a
                               posbase_pe = 10 reference model after one MaskedAdam step.

Usage:  python tests/golden/make_golden_posenc.py
"""
import os
import shutil
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402


class _posenc:
    """Inside: the reference's DirectVoxGO is built with `posbase_pe=P` (make_golden._scene has no such argument), and
    make_golden.save records P and drops the gradient of k0, which the reference leaves None."""

    def __init__(self, R, P):
        self.R, self.P = R, P

    def __enter__(self):
        # (the reference module itself is left alone: its constructor calls super(DirectVoxGO, self))
        self.module, self.save = self.R.dvgo, make_golden.save
        P, save, cls = self.P, self.save, self.module.DirectVoxGO
        seen = {}

        def build(*args, **kw):          # + a hook that keeps what the reference feeds its colour head
            m = cls(*args, posbase_pe=P, **kw)
            m.rgbnet.register_forward_pre_hook(lambda mod, inp: seen.__setitem__('head_input', inp[0].detach().clone()))
            return m
        self.R.dvgo = types.SimpleNamespace(DirectVoxGO=build)

        def save_posenc(name, **arrs):
            assert arrs.get('grad_k0') is None, 'the reference trained k0 through the posenc head'
            arrs.pop('grad_k0', None)
            save(name, posbase_pe=np.int64(P), head_input=seen['head_input'], **arrs)
        make_golden.save = save_posenc
        return self

    def __exit__(self, *exc):
        self.R.dvgo, make_golden.save = self.module, self.save
        return False


def gen_checkpoint_posenc(R, P=10):
    """make_golden.gen_checkpoint's recipe (one MaskedAdam step, then torch.save of what run.py:430-437 saves) on a
    posbase_pe model with the lego head (width 128, rgbnet_direct=True)."""
    rng = np.random.default_rng(912)
    with _posenc(R, P):
        m, mn, mx = make_golden._scene(R, rng, fine=True, nvox=10 ** 3, width=128, direct=True)
    ro, rd, vd = make_golden.lego_like_rays(R, rng, n_views=4, H=6, W=6, focal=6 * 1111.11 / 800 * 3.0, radius=3.0)
    target = torch.from_numpy(rng.random((ro.shape[0], 3)).astype(np.float32))
    rk = dict(near=0.5, far=6.0, bg=1, stepsize=0.5, inverse_y=False, flip_x=False, flip_y=False)
    groups = [{'params': m.density, 'lr': 0.1, 'skip_zero_grad': True},
              {'params': m.k0, 'lr': 0.1, 'skip_zero_grad': True},
              {'params': m.rgbnet.parameters(), 'lr': 1e-3, 'skip_zero_grad': False}]
    opt = R.masked_adam.MaskedAdam(groups)
    res = m(ro, rd, vd, global_step=1, **rk)
    opt.zero_grad(set_to_none=True)
    make_golden._loss(res, target, ro.shape[0]).backward()
    assert m.k0.grad is None
    opt.step()
    path = os.path.join(HERE, 'ref_checkpoint_posenc.tar')
    torch.save({'global_step': 1, 'model_kwargs': m.get_kwargs(), 'model_state_dict': m.state_dict(),
                'optimizer_state_dict': opt.state_dict()}, path)
    print('wrote', path, os.path.getsize(path) // 1024, 'KiB')


def main():
    R = make_golden.import_reference()
    try:
        with _posenc(R, 10):
            make_golden.gen_forward(R, fine=True, name='forward_fine_posenc', width=128, direct=True)
        with _posenc(R, 4):
            make_golden.gen_forward(R, fine=True, name='forward_fine_posenc_p4', width=128, direct=False)
        gen_checkpoint_posenc(R)
    finally:
        shutil.rmtree(R.scratch, ignore_errors=True)


if __name__ == '__main__':
    main()
