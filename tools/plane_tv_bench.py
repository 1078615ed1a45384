"""Time of the plane regulariser (csrc/plane_tv.hip, ops.plane_reg_add_grad): ONE launch over the six tensors of a
VMTriPlaneVoxGO -- three planes [1,16,S,S] and three lines [1,16,S,1], channels-last -- against what a user has without it:
  hip_one   ops.plane_reg_add_grad on the six tensors (TV on planes and lines, L1 on the lines)
  hip_3d_x6 six calls of the 3-D kernel, ops.total_variation_add_grad, on [1,C,1,H,W] views (TV only: it has no L1, and its
            line form is a view with W == 1; weights chosen so that the TV part is bit-equal to hip_one's)
  torch     the same arithmetic restated in torch ops on the same tensors (dense mode adds everywhere; sparse mode masks
            with grad != 0), L1 included
at S in {160, 320}, dense and sparse mode (sparse: about half of every gradient exactly zero).

Protocol: one process; every variant and shape warmed up; within a round the variants alternate; a timed window is `--reps`
back-to-back calls between two device events (a single call is a few microseconds of GPU work: one call per window would
time the events), reported per call; the median over rounds and the spread (max - min of the per-round values).  `host_us`
is the host clock around the same window up to the last call's return, without a synchronise: what the calls cost the
Python thread.  `GBps` is the algorithmic traffic -- 12 B per element: parameter read, gradient read and written; the four
neighbour reads are served by the caches -- over the device time; the tensors are 1.2 M floats at S = 160 and 4.9 M at 320,
cache-resident, so this is not an HBM rate.  Before timing, hip_one's result is compared with the other two on the same
inputs (TV only: bit-equal to the 3-D kernel; with L1: max |difference| to the torch restatement).
Prints one JSON line per case; `--out FILE` also writes them there.

  python tools/plane_tv_bench.py [--reps 200] [--rounds 5] [--sizes 160,320] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=200, help='calls per timed window')
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--sizes', default='160,320')
ap.add_argument('--comp', type=int, default=16)
ap.add_argument('--out', default=None)
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from directvoxgo_amd import ops  # noqa: E402

assert torch.cuda.is_available(), 'plane_tv_bench needs the GPU: a CPU run measures nothing'
W_TV_PLANE, W_TV_LINE, W_L1 = 0.75, 0.375, 0.01


def tensors(S, R, gen, sparse):
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)          # noqa: E731
    shapes = [(1, R, S, S)] * 3 + [(1, R, S, 1)] * 3
    params = [cl(torch.randn(s, generator=gen, device='cuda') * 0.5) for s in shapes]
    grads = [cl(torch.randn(s, generator=gen, device='cuda')) for s in shapes]
    if sparse:
        for g in grads:
            g[torch.rand(g.shape, generator=gen, device='cuda') < 0.5] = 0.0
    return params, grads


def weights(with_l1):
    return [(W_TV_PLANE, W_TV_PLANE, 0.0)] * 3 + [(W_TV_LINE, 0.0, W_L1 if with_l1 else 0.0)] * 3


def hip_one(params, grads, dense, with_l1=True):
    ops.plane_reg_add_grad(params, grads, weights(with_l1), dense)


def hip_3d_x6(params, grads, dense):
    for i, (p, g) in enumerate(zip(params, grads)):
        w = 6 * (W_TV_PLANE if i < 3 else W_TV_LINE)          # the 3-D kernel divides by 6
        ops.total_variation_add_grad(p.unsqueeze(2), g.unsqueeze(2), w, w, w, dense)


def torch_restatement(params, grads, dense, with_l1=True):
    for (wh, ww, wl1), p, g in zip(weights(with_l1), params, grads):
        t = torch.zeros_like(p)
        if p.shape[3] > 1:
            d = (p[..., 1:] - p[..., :-1]).clamp(-1, 1) * ww
            t[..., 1:] += d
            t[..., :-1] -= d
        d = (p[:, :, 1:] - p[:, :, :-1]).clamp(-1, 1) * wh
        t[:, :, 1:] += d
        t[:, :, :-1] -= d
        if wl1 != 0:
            t += wl1 * torch.sign(p)
        if not dense:
            t *= (g != 0)
        g += t


def window(fn, params, grads, dense, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(reps):
        fn(params, grads, dense)
    b.record()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps, host * 1e6 / reps          # microseconds per call: device, host


VARIANTS = {'hip_one': hip_one, 'hip_3d_x6': hip_3d_x6, 'torch': torch_restatement}
rows = [{'reps': args.reps, 'rounds': args.rounds, 'comp': args.comp, 'device': torch.cuda.get_device_name(0)}]
print(json.dumps(rows[0]), flush=True)
gen = torch.Generator(device='cuda').manual_seed(0)
for S in [int(v) for v in args.sizes.split(',')]:
    for dense in (True, False):
        params, grads = tensors(S, args.comp, gen, sparse=not dense)
        elements = sum(p.numel() for p in params)
        # same results first: TV only against the 3-D kernel (bits), everything against the torch restatement (values)
        a, b = [g.clone() for g in grads], [g.clone() for g in grads]
        hip_one(params, a, dense, with_l1=False)
        hip_3d_x6(params, b, dense)
        bit_equal = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
        a, b = [g.clone() for g in grads], [g.clone() for g in grads]
        hip_one(params, a, dense)
        torch_restatement(params, b, dense)
        max_diff = max(float((x - y).abs().max()) for x, y in zip(a, b))
        del a, b
        work = {v: [g.clone() for g in grads] for v in VARIANTS}          # each variant accumulates into its own copies
        for v, fn in VARIANTS.items():
            window(fn, params, work[v], dense, 20)
        dev = {v: [] for v in VARIANTS}
        host = {v: [] for v in VARIANTS}
        for _ in range(args.rounds):
            for v, fn in VARIANTS.items():
                d, h = window(fn, params, work[v], dense, args.reps)
                dev[v].append(d); host[v].append(h)
        row = {'S': S, 'dense_mode': dense, 'elements': elements, 'tv_bit_equal_to_3d_kernel': bit_equal,
               'max_abs_diff_to_torch': max_diff}
        for v in VARIANTS:
            med = float(np.median(dev[v]))
            row[v] = {'device_us': round(med, 2), 'spread_us': round(max(dev[v]) - min(dev[v]), 2),
                      'host_us': round(float(np.median(host[v])), 2), 'GBps': round(12.0 * elements / (med * 1e-6) / 1e9, 1)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del params, grads, work
        torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        for r in rows:
            fh.write(json.dumps(r) + '\n')
