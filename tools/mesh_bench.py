"""Mesh extraction (csrc/mesh.hip, export.extract_mesh) on the synthetic scene (scenes.synthetic_scene, blob density and
its occupancy mask): the density grid's own lattice at 160^3 and 256^3, and the 256^3 grid resampled to 512^3.  One JSON
line per case:

  extract_ms          extract_mesh with colours (field, count + scan, the 8-byte (V, F) read, emit, colour head): host
                      clock around synchronised work, warmed up, mean of --reps
  extract_ms_nocolor  the same without the colour head
  V, F                vertices and faces
  bytes               what the passes must move at least, from the shapes (pass_bytes)
  oracle_ms           the numpy statement (tests/mesh_oracle.py: lattice_field + marching_tets) on the host, one run;
                      null where it was not run (--oracle-max-points)

Kernel times come from a separate run per case under the kernel tracer (--trace: the extractions only):
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/mesh_bench.py --trace --cases 256
and are set against each pass's HBM floor, pass_bytes over the 8 TB/s peak (MI355X_MICROARCH), in DESIGN.md 6c.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

CASES = {'160': (160, None), '256': (256, None), '256to512': (256, 512)}


def pass_bytes(grid, R, V, F, copy):
    """least HBM traffic per pass (every array touched once; neighbour reads are assumed to hit L1/L2):
    field: density (the copied voxels, or the whole grid when sampling) + mask bytes read, the padded field written;
    count: field read, crossing masks written; emit_vertices: masks read, 24 B per vertex written;
    emit_faces: field and masks read, 12 B per face written."""
    P = int(np.prod([r + 2 for r in R]))
    G = int(np.prod(grid))
    src = int(np.prod(R)) if copy else G
    return {'field': 4 * src + G + 4 * P, 'count': 4 * P + P, 'emit_vertices': P + 24 * V,
            'emit_faces': 4 * P + P + 12 * F}


def scene_model(world):
    import torch
    from directvoxgo_amd.dvgo import DirectVoxGO
    from directvoxgo_amd.scenes import synthetic_scene
    sc = synthetic_scene(world=world, n_rays=16, device='cuda')
    m = DirectVoxGO(sc['xyz_min'].cpu(), sc['xyz_max'].cpu(), num_voxels=world ** 3, num_voxels_base=world ** 3,
                    alpha_init=1e-2, rgbnet_dim=12).cuda()
    with torch.no_grad():
        m.density.copy_(sc['density']); m.k0.copy_(sc['k0']); m.mask_cache.mask.copy_(sc['mask'])
    return m


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.mean(ts)), 1e3 * float(np.std(ts)), out


def run_case(name, reps, oracle_max_points, trace):
    import torch
    from directvoxgo_amd.export import extract_mesh, lattice, mesh_field
    world, res = CASES[name]
    m = scene_model(world)
    kw = {} if res is None else {'resolution': res}
    if trace:
        for _ in range(reps):
            extract_mesh(m, 0.5, **kw)
        torch.cuda.synchronize()
        return None
    ms, sd, mesh = timed(lambda: extract_mesh(m, 0.5, **kw), reps)
    ms_nc, sd_nc, _ = timed(lambda: extract_mesh(m, 0.5, color=False, **kw), reps)
    lat = lattice(m, **kw)
    V, F = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    out = {'case': name, 'grid': world, 'lattice': list(lat.R), 'V': V, 'F': F, 'extract_ms': round(ms, 2),
           'extract_ms_sd': round(sd, 2), 'extract_ms_nocolor': round(ms_nc, 2), 'extract_ms_nocolor_sd': round(sd_nc, 2),
           'bytes': pass_bytes((world,) * 3, lat.R, V, F, lat.copy), 'oracle_ms': None}
    P = int(np.prod([r + 2 for r in lat.R]))
    if P <= oracle_max_points:
        import mesh_oracle as M
        field, iso, _ = mesh_field(m, 0.5, **kw)
        mc = m.mask_cache
        dens = m.density.detach()[0, 0].cpu().numpy()
        args = dict(mask=mc.mask.cpu().numpy(), mask_scale=mc.xyz2ijk_scale.cpu().numpy(),
                    mask_shift=mc.xyz2ijk_shift.cpu().numpy(), copy=lat.copy)
        t0 = time.perf_counter()
        Fh = M.lattice_field(dens, lat.R, lat.a, lat.s, lat.mn, lat.h, iso, **args)
        v, f, _ = M.marching_tets(Fh, iso, lat.mn, lat.h)
        out['oracle_ms'] = round(1e3 * (time.perf_counter() - t0), 1)
        out['oracle_matches_counts'] = bool(len(v) == V and len(f) == F)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='160,256,256to512')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--oracle-max-points', type=int, default=258 ** 3)
    ap.add_argument('--trace', action='store_true', help='run the extractions only (under rocprofv3)')
    ap.add_argument('--out', default=None, help='also write the JSON lines to this file')
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'mesh_bench needs a GPU'
    lines = []
    for name in args.cases.split(','):
        r = run_case(name, args.reps, args.oracle_max_points, args.trace)
        if r is not None:
            print(json.dumps(r), flush=True)
            lines.append(r)
    if args.out and lines:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(json.dumps(r) for r in lines) + '\n')


if __name__ == '__main__':
    main()
