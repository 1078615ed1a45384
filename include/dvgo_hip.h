/*
 * dvgo_hip.h -- C ABI of libdvgo_hip.so, the MI355X (gfx950) implementation of
 * DirectVoxGO's volumetric ray-marching hot path.
 *
 * This is the drop-in boundary.  The reference binds this path through a pybind11
 * module (`render_utils_cuda`, /root/reference/lib/cuda/render_utils.cpp:144-155) plus
 * two third-party calls (torch F.grid_sample, torch_scatter.segment_coo).  Every entry
 * point below replaces one of those callables; the reference file:line is cited on each.
 * The ctypes binding a maintainer would add is shown in INTEGRATION.md and implemented in
 * directvoxgo_amd/_lib.py + directvoxgo_amd/render_utils.py.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless it is
 *     documented as host; no torch / ATen types.
 *   - fp32 tensors (`float`), int64 indices (`int64_t`), bool tensors as 1 byte/element
 *     (`uint8_t`, 0/1) -- the dtypes the reference uses in practice.
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing
 *     synchronises unless stated.  (The reference uses the legacy default stream and
 *     the current device; callers here pass torch's current stream.)
 *   - return value: 0 on success, otherwise the hipError_t of the failed launch /
 *     a negative DVGO_E* code for invalid arguments.  Empty inputs (0 rays / 0 points)
 *     are valid everywhere and return 0 without launching.
 *   - outputs are caller-allocated; sizes are stated per function.
 *   - `m_dev` (where an entry point has it, right after a sample count M): NULL, or a DEVICE pointer to the actual
 *     sample count.  The kernels then process min(M, *m_dev) samples and M is only the capacity of the arrays: the
 *     training step keeps the data-dependent count of surviving samples on the device and never reads it back
 *     (train.py, fused.py `capacity` mode), which removes the forward's host synchronisation.
 */
#ifndef DVGO_HIP_H
#define DVGO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVGO_EINVAL (-1)   /* invalid argument (null pointer, negative size, bad stride) */
#define DVGO_ERANGE (-2)   /* size exceeds what the kernel's 32-bit indexing supports    */

/* version of this ABI; bumped on any signature change (6: the positional-encoding colour head; 7: the contracted
 * sampler and the distortion loss of unbounded scenes; 8: the tri-plane sampler; 9: the trilinear sample's gradient
 * with respect to the position; 10: the LIIF plane decoder; 11: the fused march's gradient with respect to its rays).
 * The two dvgo_plane_rows_*, the two dvgo_vm_*, the two dvgo_hash_*, the two dvgo_vm_density_*, the two dvgo_march_vm_density*, the two dvgo_march_contract_density*, the dvgo_contract_positions, the two dvgo_contract_ray_bwd* and the dvgo_hash_bwd_xyz entries were added without a bump, unlike the additions before them (the two dvgo_vm_*bwd_xyz entries were added the same way): an
 * existing test pins the value 11, and a library built before them is still caught at load, by the check that every declared entry is exported. */
#define DVGO_ABI_VERSION 11
int dvgo_abi_version(void);

/* Kernel-variant selection for A/B measurements (process-global; defaults are the fastest
 * measured variants).  key: one of DVGO_TUNE_*; returns DVGO_EINVAL for an unknown key. */
#define DVGO_TUNE_FEAT_BWD    0   /* 0 = one atomic per (sample,corner,channel); 1 = LDS de-duplicated rows */
#define DVGO_TUNE_DENSITY_BWD 1   /* 0 = direct atomics; 1 = LDS de-duplicated */
#define DVGO_TUNE_DENSITY_FWD 2   /* march_density: 1 = corner loads in flight together as z-pairs + occupancy byte a chunk ahead; 0 = round 2's body */
#define DVGO_TUNE_GATHER      3   /* march_gather: 1 = corner rows requested four at a time; 0 = one corner per round trip */
#define DVGO_TUNE_EXPERIMENT  4   /* march_density timing experiments (bit mask, results wrong when non-zero; tools/fwd_ab.py) */
#define DVGO_TUNE_COUNT       8
int dvgo_set_tuning(int key, int value);

/* ---------------------------------------------------------------------------------
 * Sampling helpers.  render_utils.cpp:44-65 / render_utils_kernel.cu:11-132 (K1-K3)
 * --------------------------------------------------------------------------------- */
/* infer_t_minmax(rays_o, rays_d, xyz_min, xyz_max, near, far) -> [t_min, t_max]   [n_rays] each */
int dvgo_infer_t_minmax(const float* rays_o, const float* rays_d,
                        const float* xyz_min, const float* xyz_max,
                        float near, float far, int64_t n_rays,
                        float* t_min, float* t_max, void* stream);

/* infer_n_samples(t_min, t_max, stepdist) -> n_samples [n_rays] int64 */
int dvgo_infer_n_samples(const float* t_min, const float* t_max, float stepdist,
                         int64_t n_rays, int64_t* n_samples, void* stream);

/* infer_ray_start_dir(rays_o, rays_d, t_min) -> [rays_start, rays_dir]   [n_rays,3] each */
int dvgo_infer_ray_start_dir(const float* rays_o, const float* rays_d, const float* t_min,
                             int64_t n_rays, float* rays_start, float* rays_dir, void* stream);

/* ---------------------------------------------------------------------------------
 * sample_pts_on_rays.  render_utils.cpp:67-78 / render_utils_kernel.cu:138-236 (K4-K6)
 * The output length M0 = sum(N_steps) is data dependent, so the op is two-phase:
 *   1. dvgo_sample_pts_prepare : K1+K2+K3 and the inclusive cumsum of N_steps.
 *      The caller reads n_steps_cumsum[n_rays-1] (one D2H copy: the reference's own
 *      `N_steps.sum().item()`, :206) and allocates the M0-sized outputs.
 *   2. dvgo_sample_pts_fill    : ray_id / step_id / rays_pts / mask_outbbox.
 * --------------------------------------------------------------------------------- */
int dvgo_sample_pts_prepare(const float* rays_o, const float* rays_d,
                            const float* xyz_min, const float* xyz_max,
                            float near, float far, float stepdist, int64_t n_rays,
                            float* t_min, float* t_max,            /* [n_rays]         */
                            int64_t* n_steps,                      /* [n_rays]         */
                            int64_t* n_steps_cumsum,               /* [n_rays] inclusive */
                            float* rays_start, float* rays_dir,    /* [n_rays,3]       */
                            void* stream);

int dvgo_sample_pts_fill(const float* rays_start, const float* rays_dir,
                         const float* xyz_min, const float* xyz_max,
                         const int64_t* n_steps_cumsum, int64_t n_rays,
                         float stepdist, int64_t total_len,        /* M0               */
                         float* rays_pts,                          /* [M0,3]           */
                         uint8_t* mask_outbbox,                    /* [M0]             */
                         int64_t* ray_id, int64_t* step_id,        /* [M0]             */
                         void* stream);

/* sample_ndc_pts_on_rays.  render_utils.cpp:80-91 / render_utils_kernel.cu:238-287 (K7)
 * -> rays_pts [n_rays,N_samples,3], mask_outbbox [n_rays,N_samples] */
int dvgo_sample_ndc_pts_on_rays(const float* rays_o, const float* rays_d,
                                const float* xyz_min, const float* xyz_max,
                                int n_samples, int64_t n_rays,
                                float* rays_pts, uint8_t* mask_outbbox, void* stream);

/* ---------------------------------------------------------------------------------
 * maskcache_lookup.  render_utils.cpp:93-102 / render_utils_kernel.cu:300-351 (K8)
 * world [sz_i,sz_j,sz_k] bool, xyz [n_pts,3] -> out [n_pts] bool (fully written)
 * --------------------------------------------------------------------------------- */
int dvgo_maskcache_lookup(const uint8_t* world, const float* xyz,
                          const float* xyz2ijk_scale, const float* xyz2ijk_shift,
                          int sz_i, int sz_j, int sz_k, int64_t n_pts,
                          uint8_t* out, void* stream);

/* ---------------------------------------------------------------------------------
 * raw2alpha / raw2alpha_backward.  render_utils.cpp:104-114 / _kernel.cu:357-428 (K9,K10)
 * --------------------------------------------------------------------------------- */
int dvgo_raw2alpha(const float* density, float shift, float interval, int64_t n_pts,
                   float* exp_d, float* alpha, void* stream);
int dvgo_raw2alpha_backward(const float* exp_d, const float* grad_back, float interval,
                            int64_t n_pts, float* grad, void* stream);

/* ---------------------------------------------------------------------------------
 * alpha2weight / alpha2weight_backward.  render_utils.cpp:116-141 / _kernel.cu:430-561
 * (K11-K13).  ray_id must be segment-contiguous (as the reference requires).
 * Outputs of alpha2weight: weight,T [n_pts]; alphainv_last [n_rays]; i_start,i_end [n_rays].
 * All outputs are fully written (the pre-fills of :478-482 are done here).
 * The transmittance recurrence is evaluated in the reference's serial order and
 * precision, so results are bit-identical to the oracle for identical inputs.
 * --------------------------------------------------------------------------------- */
int dvgo_alpha2weight(const float* alpha, const int64_t* ray_id, int64_t n_pts, int64_t n_rays,
                      float* weight, float* T, float* alphainv_last,
                      int64_t* i_start, int64_t* i_end, void* stream);
int dvgo_alpha2weight_backward(const float* alpha, const float* weight, const float* T,
                               const float* alphainv_last, const int64_t* i_start,
                               const int64_t* i_end, int64_t n_rays, int64_t n_pts,
                               const float* grad_weights, const float* grad_last,
                               float* grad /* [n_pts], fully written */, void* stream);

/* ---------------------------------------------------------------------------------
 * Trilinear grid interpolation ("DenseGrid").  Replaces
 *   lib/dvgo.py:312-328 grid_sampler -> F.grid_sample(grid[1,C,X,Y,Z], ind_norm,
 *   mode='bilinear', align_corners=True)  and its autograd backward w.r.t. the grid.
 * The grid is addressed through ELEMENT strides (sC,sX,sY,sZ) so the reference layout
 * [1,C,X,Y,Z] (sZ=1) and the channels-last layout this library prefers (sC=1) are both
 * accepted.  xyz [M,3] world coordinates; out / grad_out are [M,C] row-major.
 * grad_grid must be zero-initialised (or hold a partial sum) -- values are accumulated
 * with float atomics, so the summation order is not reproducible (neither is the
 * reference's, run.py:147-149).
 * --------------------------------------------------------------------------------- */
int dvgo_grid_sample_fwd(const float* grid, int C, int X, int Y, int Z,
                         int64_t sC, int64_t sX, int64_t sY, int64_t sZ,
                         const float* xyz, const float* xyz_min, const float* xyz_max,
                         int64_t M, float* out, void* stream);
int dvgo_grid_sample_bwd(const float* grad_out, int C, int X, int Y, int Z,
                         int64_t sC, int64_t sX, int64_t sY, int64_t sZ,
                         const float* xyz, const float* xyz_min, const float* xyz_max,
                         int64_t M, float* grad_grid, void* stream);

/* ---------------------------------------------------------------------------------
 * segment sum.  Replaces torch_scatter.segment_coo(src, index, out, reduce='sum')
 * (lib/dvgo.py:554-559,571-575).  src [M,C], index [M] int64 sorted/segment-contiguous,
 * out [N,C] accumulated into (caller zero-fills, as the reference passes out=zeros).
 * --------------------------------------------------------------------------------- */
int dvgo_segment_sum(const float* src, const int64_t* index, int64_t M, int C,
                     int64_t N, float* out, void* stream);

/* ---------------------------------------------------------------------------------
 * Fused march (the MI355X-native fast path behind DirectVoxGO.forward, lib/dvgo.py:450-577).
 * See DESIGN.md "Fused pipeline" for the data flow.  N rays; the per-ray inputs n_steps /
 * rays_start / rays_dir come from dvgo_sample_pts_prepare (n_steps_cumsum may be NULL there).
 *
 * In the dvgo_march_* entry points xyz_min, xyz_max, xyz2ijk_scale and xyz2ijk_shift are
 * HOST pointers to 3 floats (model constants; they travel as kernel arguments).
 *
 * `stepdist` > 0 : metric spacing, sample s of ray r sits at rays_start[r] + rays_dir[r]*(stepdist*s)
 *                  (K6, render_utils_kernel.cu:178-181; rays_start/rays_dir from dvgo_sample_pts_prepare).
 * `stepdist` < 0 : NDC / MPI spacing with N_samples-1 = -stepdist: rays_o[r] + rays_d[r]*((float)s/(N_samples-1))
 *                  (K7, render_utils_kernel.cu:254-257; pass rays_o / rays_d and n_steps[r] = N_samples).
 *
 * Scratch records.  Each ray owns a slice of the rec2/rec3 scratch arrays that starts at
 *   n_steps_cumsum[r] - n_steps[r]   when n_steps_cumsum != NULL (exact, M0 records in total), or
 *   r * rec_stride                   when n_steps_cumsum == NULL (rec_stride >= max n_steps; since
 *                                    t is clamped to [near,far], ceil((far-near)/stepdist)+1 is a
 *                                    bound -- saves the scan and the host read of M0).
 *
 * dvgo_march_density: one wavefront per ray.  sample -> bbox test -> mask lookup ->
 *   density trilinear -> raw2alpha -> alpha>thres filter -> transmittance scan with early
 *   stop (T<1e-3) -> weight>thres filter (both filters only when fast_color_thres > 0,
 *   lib/dvgo.py:478,488).  Writes per ray r:
 *     rec2[base+j] (j < n2[r]) : {step, exp_d, alpha, T_before} of the j-th sample that entered
 *                                compositing (post alpha filter, up to and including the early-stop
 *                                sample); step has bit 31 set when the sample also passed the
 *                                weight filter
 *   and n2[r] (records of the ray), n3[r] (how many of them passed the weight filter: the reference's final
 *   sample set), alphainv_last[r].  mask may be NULL (no occupancy skipping).
 * --------------------------------------------------------------------------------- */
typedef struct { int32_t step; float exp_d; float alpha; float T; } dvgo_rec2_t;     /* 16 B */

int dvgo_march_density(float* rays_start, float* rays_dir,
                       int64_t* n_steps, const int64_t* n_steps_cumsum, int64_t rec_stride,
                       int64_t n_rays,
                       const float* xyz_min, const float* xyz_max, float stepdist,
                       const uint8_t* mask, int mX, int mY, int mZ,
                       const float* xyz2ijk_scale, const float* xyz2ijk_shift,
                       const float* density, int X, int Y, int Z,            /* [X,Y,Z] contiguous */
                       float act_shift, float interval, float fast_color_thres,
                       dvgo_rec2_t* rec2,
                       int32_t* n2, int32_t* n3, float* alphainv_last,
                       int32_t* brick_cnt /* NULL, or [dvgo_n_bricks(X,Y,Z)] zero-initialised counters: the samples
                                             that entered compositing are counted per brick for the backward's
                                             owner-computes scatter (see "Brick scatter" below) */,
                       const float* rays_o, const float* rays_d, float near, float far
                                          /* rays_o != NULL (fixed-stride records, stepdist > 0): K1-K3 of
                                             dvgo_sample_pts_prepare are computed by this launch and rays_start / rays_dir /
                                             n_steps are OUTPUTS; NULL: they are inputs */,
                       int32_t* tail_ticket /* NULL, or one zero-initialised int32 (left at zero): the LAST workgroup to finish
                                               also does the work of dvgo_march_scans -- off3 [n_rays + 1] = exclusive scan of
                                               n3 and, when brick_cnt and brick_off are given, the brick tables -- so that no
                                               scan launch is needed between this call and dvgo_march_gather.  One call at a
                                               time per ticket word. */,
                       int64_t* off3, int n_bricks, int32_t* brick_off, int32_t* brick_cursor, int32_t* extra_off,
                       int32_t* active, int32_t* extra_brick, int n_extra_max, int slice_len,
                       void* stream);

/* dvgo_march_hit: hit[r] = 1 iff ray r has an in-box sample whose nearest occupancy voxel is set -- the fused
 *   form of DirectVoxGO.hit_coarse_geo (lib/dvgo.py:412-423), one wavefront per ray.  Host pointers as above. */
int dvgo_march_hit(const float* rays_start, const float* rays_dir, const int64_t* n_steps, int64_t n_rays,
                   const float* xyz_min, const float* xyz_max, float stepdist,
                   const uint8_t* mask, int mX, int mY, int mZ,
                   const float* xyz2ijk_scale, const float* xyz2ijk_shift, uint8_t* hit, void* stream);

/* exclusive scan of int32 counts -> int64 offsets [n+1] (offsets[n] = total) */
int dvgo_exclusive_scan_i32(const int32_t* counts, int64_t n, int64_t* offsets, void* stream);

/* dvgo_march_gather: one wavefront per ray over its rec2 records; the records flagged as kept are compacted to
 *   [off3[r], off3[r+1]) (ray-major, the reference's order; off3 = exclusive scan of n3, M3 = off3[N]).  Writes
 *   ray_id, step_id [M3] int64; weights (= T * alpha), alpha [M3]; k0 features [M3,C] trilinearly interpolated from
 *   the feature grid (element strides as dvgo_grid_sample_fwd). */
int dvgo_march_gather(const dvgo_rec2_t* rec2, const int32_t* n2, const int64_t* n_steps, const int64_t* n_steps_cumsum,
                      int64_t rec_stride, const int64_t* off3, int64_t n_rays, int64_t M3,
                      const float* rays_start, const float* rays_dir, float stepdist,
                      const float* xyz_min, const float* xyz_max,
                      const float* k0, int C, int X, int Y, int Z,
                      int64_t sC, int64_t sX, int64_t sY, int64_t sZ,
                      int64_t* ray_id, int64_t* step_id, float* weights, float* alpha,
                      float* feat, void* stream);

/* dvgo_march_composite: rgb_marched[r] = sum_k w*rgb + alphainv_last[r]*bg ; optional depth
 *   = sum_k w*step_id (lib/dvgo.py:554-576).  One wavefront per ray over [off3[r], off3[r+1]). */
int dvgo_march_composite(const float* weights, const float* rgb /* [M3,3] */,
                         const int64_t* step_id, const int64_t* off3, int64_t n_rays,
                         const float* alphainv_last, float bg,
                         float* rgb_marched /* [N,3] */, float* depth /* [N] or NULL */,
                         void* stream);

/* Backward of the composite w.r.t. weights and rgb (either output may be NULL):
 *   grad_weights[i] = sum_c g[r,c]*rgb[i,c] ; grad_rgb[i,c] = g[r,c]*weights[i], r = ray_id[i].
 *   grad_last (NULL or [n_rays]) = bg * sum_c g[r,c], the gradient w.r.t. alphainv_last (lib/dvgo.py:559),
 *   written by the same launch.  accumulate != 0: grad_rgb and grad_last already hold the gradient of the same two
 *   tensors through another consumer (the loss's rgbper and entropy terms, run.py:381-385) and are added to. */
int dvgo_march_composite_bwd(const float* grad_rgb_marched /* [N,3] */, const float* weights,
                             const float* rgb, const int64_t* ray_id, int64_t M3, const int64_t* m_dev, int64_t n_rays,
                             float bg, float* grad_weights /* [M3] */, float* grad_rgb /* [M3,3] */,
                             float* grad_last, int accumulate, void* stream);

/* dvgo_march_feat_bwd: scatter grad_feat [M3,C] into grad_k0 (float atomics, de-duplicated per wavefront in LDS;
 *   element strides sC,sX,sY,sZ of the destination).
 *   grad_extra (NULL or [M3]): one more per-sample scalar scattered with the same trilinear weights as channel C
 *   of the same voxel row -- used with a combined gradient buffer of 64-byte rows (sC = 1, sZ = 16 floats: 12
 *   feature channels, the density gradient, 3 pad): float atomics are bound by 64-B requests, an aligned row is
 *   exactly one, and the density gradient of the kept samples then costs no request of its own.  Needs
 *   C == 12 and a row layout with sZ > C, else DVGO_ERANGE. */
int dvgo_march_feat_bwd(const float* grad_feat, const float* grad_extra, const int64_t* ray_id, const int64_t* step_id,
                        int64_t M3, const float* rays_start, const float* rays_dir, float stepdist,
                        const float* xyz_min, const float* xyz_max,
                        int C, int X, int Y, int Z, int64_t sC, int64_t sX, int64_t sY, int64_t sZ,
                        float* grad_k0, void* stream);

/* dvgo_march_density_bwd: one wavefront per ray.  alpha2weight backward (K13) over the rec2
 *   samples, raw2alpha backward (K10), then the trilinear scatter into grad_density (voxel v at
 *   grad_density[v * grad_stride]; 1 for the plain [X,Y,Z] grid).
 *   grad_weights is indexed in the M3 order of dvgo_march_gather; grad_last may be NULL (= 0).
 *   grad_kept (NULL or [M3]): when given, the samples kept by dvgo_march_gather write their density gradient there
 *   (for dvgo_march_feat_bwd's grad_extra) instead of scattering it; only the dropped ones are scattered here.
 *   brick_cursor (NULL or [n_bricks], from dvgo_brick_scan): when given nothing is scattered here (grad_density and
 *   grad_kept are ignored): every sample is appended to the list of each brick it touches -- brick_recs[slot] =
 *   {int32 kept index in the M3 order or -1, int32 ray, int32 step, float density gradient} (16 B) -- for
 *   dvgo_brick_accumulate. */
int dvgo_march_density_bwd(const dvgo_rec2_t* rec2, const int32_t* n2, const int64_t* n_steps,
                           const int64_t* n_steps_cumsum, int64_t rec_stride, const int64_t* off3,
                           int64_t n_rays,
                           const float* rays_start, const float* rays_dir, float stepdist,
                           const float* xyz_min, const float* xyz_max,
                           const float* alphainv_last, float interval,
                           const float* grad_weights /* [M3] */, const float* grad_last /* [N] */,
                           int X, int Y, int Z, float* grad_density, int64_t grad_stride, float* grad_kept,
                           int32_t* brick_cursor, void* brick_recs,
                           void* stream);

/* dvgo_march_ray_bwd: the gradient of the fused march with respect to its RAYS (csrc/march_raygrad.hip; DESIGN.md section 6h;
 *   camera-pose refinement on the fused path).  One wavefront per ray; metric steps only
 *   (stepdist > 0: NDC spacing is not differentiated).
 *   rec2 .. alphainv_last, interval, grad_weights, grad_last: as dvgo_march_density_bwd, from the same forward.  The walk
 *   is that kernel's: chunks of 64 records from the far end, and per record the same g_d (K13 in double, dvgo_pow_neg, the
 *   three double multiplies, narrowed once) and the same position p = fmaf(rays_dir, dist, rays_start), dist = stepdist *
 *   step, with the same bits.
 *   rays_o, rays_d [N,3], near, far: what dvgo_march_density's ray setup read; t_min and |d| = sqrtf(fmaf(dz, dz, fmaf(dy,
 *   dy, dx * dx))) are recomputed from them by the same expressions.
 *   density [X,Y,Z] contiguous; k0 with C channels and its four ELEMENT strides (as dvgo_march_gather); grad_feat [M3,C]
 *   row-major in the M3 order of dvgo_march_gather, or NULL: no feature term.  grad_weights may be NULL when M3 == 0.
 *   The grids must hold what the forward read: launch this before anything that updates them in place.
 *   Per record, with the cell, the per-axis weights and the in-range test of the gather, and the corner chains of
 *   dvgo_grid_sample_bwd_xyz (n = 0..7, corners outside skipped, each chain from 0):
 *       dX = chain over the density grid;  ax = fmaf(g_d, dX, 0);  likewise ay, az
 *       for a record kept by dvgo_march_gather (index i in the M3 order), when grad_feat is given, c ascending:
 *           dX_c = chain over k0 channel c;  ax = fmaf(grad_feat[i * C + c], dX_c, ax);  likewise ay, az
 *       g_p = (ax * ((float)(X-1) / (xyz_max[0] - xyz_min[0])), ay * ..., az * ...)
 *       lam = t_min + dist / |d|
 *   A record with g_d == 0 and no feature term contributes exact zeros.  Per ray, in float32 and in a fixed order (per
 *   chunk a butterfly over the 64 lanes, lanes without a record adding 0; chunks far to near into one accumulator):
 *       grad_o[ray] = sum g_p          grad_d[ray] = sum (lam * g_p)
 *   Every ray < n_rays is written with plain stores by one lane, zeros for a ray without records: no atomics, no
 *   workspace, nothing to zero beforehand, bitwise repeatable.  Channels-last k0 with C % 4 == 0 and 16-byte aligned k0
 *   and grad_feat reads 16-byte vectors; everything else goes through the element strides.
 *   n_rays == 0: no-op.  DVGO_EINVAL: negative n_rays or C, an axis < 1, stepdist <= 0, null required pointers, neither
 *   n_steps_cumsum nor rec_stride > 0.  DVGO_ERANGE: n_rays * 64 >= 2^31. */
int dvgo_march_ray_bwd(const dvgo_rec2_t* rec2, const int32_t* n2, const int64_t* n_steps,
                       const int64_t* n_steps_cumsum, int64_t rec_stride, const int64_t* off3, int64_t n_rays,
                       const float* rays_start, const float* rays_dir, float stepdist,
                       const float* xyz_min, const float* xyz_max, const float* alphainv_last, float interval,
                       const float* rays_o, const float* rays_d, float near, float far,
                       const float* density, int X, int Y, int Z,
                       const float* k0, int C, int64_t sC, int64_t sX, int64_t sY, int64_t sZ,
                       const float* grad_weights /* [M3] */, const float* grad_last /* [N] */,
                       const float* grad_feat /* [M3,C] */, float* grad_o, float* grad_d, void* stream);

/* dvgo_march_ray_bwd_pts: dvgo_march_ray_bwd for a march that hands its caller the kept samples' POSITIONS in place of k0
 *   features (fused_march(positions=True): HashVoxGO, VMTriPlaneVoxGO; csrc/march_raygrad.hip).
 *   Added without a bump of DVGO_ABI_VERSION.  Every argument up to Z as in dvgo_march_ray_bwd, from the same forward; both
 *   record layouts (n_steps_cumsum, or rec_stride > 0); grad_last [N] or NULL; grad_weights may be NULL when M3 == 0.
 *   grad_pts [M3,3] row-major in the M3 order of dvgo_march_gather: the gradient that arrived for the positions, or NULL: no
 *   second term.  The walk, g_d, the position p, the cell, the weights, the in-range test and the density chain are
 *   dvgo_march_ray_bwd's (the same functions: csrc/march_records.h, csrc/xyz_corners.h).  Per record:
 *       dX = chain over the density grid;  ax = fmaf(g_d, dX, 0);  likewise ay, az
 *       g_p = (ax * ((float)(X-1) / (xyz_max[0] - xyz_min[0])), ay * ..., az * ...)
 *       for a record kept by dvgo_march_gather (index i in the M3 order), when grad_pts is given:
 *           g_p = g_p + grad_pts[3 i .. 3 i + 2]                     one float32 addition per component
 *       lam = t_min + dist / |d|
 *   A record with g_d == 0 and no pts term loads nothing and contributes exact zeros.  Per ray, dvgo_march_ray_bwd's sums in
 *   its order:  grad_o[ray] = sum g_p,  grad_d[ray] = sum (lam * g_p);  every ray < n_rays written with plain stores by one
 *   lane, zeros for a ray without records; no atomics, no LDS, no workspace, bitwise repeatable.  With grad_pts NULL the result
 *   has the bits of dvgo_march_ray_bwd called with C = 0 and grad_feat NULL.
 *   n_rays == 0: no-op, no pointer looked at.  DVGO_EINVAL: negative n_rays, an axis < 1, stepdist <= 0, then null required
 *   pointers, neither n_steps_cumsum nor rec_stride > 0.  DVGO_ERANGE: n_rays * 64 >= 2^31. */
int dvgo_march_ray_bwd_pts(const dvgo_rec2_t* rec2, const int32_t* n2, const int64_t* n_steps,
                           const int64_t* n_steps_cumsum, int64_t rec_stride, const int64_t* off3, int64_t n_rays,
                           const float* rays_start, const float* rays_dir, float stepdist,
                           const float* xyz_min, const float* xyz_max, const float* alphainv_last, float interval,
                           const float* rays_o, const float* rays_d, float near, float far,
                           const float* density, int X, int Y, int Z,
                           const float* grad_weights /* [M3] */, const float* grad_last /* [N] */,
                           const float* grad_pts /* [M3,3] or NULL */, float* grad_o, float* grad_d, void* stream);

/* ---------------------------------------------------------------------------------
 * Brick scatter: the grid-gradient sums of grid_sampler_3d_backward (behind lib/dvgo.py:321; 8*C float atomics per
 * sample in the reference) without atomics.  The lattice is cut into 8x8x8-voxel bricks; a workgroup owns one brick,
 * sums the contributions of the samples listed for it and either writes the dense gradients with plain stores
 * (every voxel of the grid is written: zeros where no sample came by) or applies the Adam update in place.
 *   dvgo_n_bricks        number of bricks of an [X,Y,Z] lattice
 *   dvgo_brick_scan      counts [n] -> offsets [n+1] (offsets[n] = number of list entries E) and fill cursors [n]
 *   dvgo_brick_accumulate
 *     brick_off [n+1]; recs [E] 16-byte records as written by dvgo_march_density_bwd; rays_start / rays_dir /
 *     stepdist / xyz_min / xyz_max (host) as given to dvgo_march_density (sample positions are rebuilt from the
 *     records' ray and step); grad_feat [M3,C] (the gradient w.r.t. the gathered features); density and k0 share the
 *     lattice, k0 channels-last.
 *     p_k0 == NULL : writes grad_k0 [X,Y,Z,C] (channels-last) and grad_density [X,Y,Z], all of both.
 *     p_k0 != NULL : MaskedAdam in place on (p, exp_avg, exp_avg_sq) of k0 and density
 *                    (adam_upd_cuda.adam_upd / masked_adam_upd, lib/cuda/adam_upd.cpp:36-68; step sizes bias-corrected
 *                    on the host as adam_upd_kernel.cu:72; masked_* = skip elements whose gradient is exactly 0);
 *                    voxels of bricks no sample touched are left alone either way (their gradient is zero: the masked
 *                    update skips them; for an unmasked group use the dense path).
 *     Built for C in {3, 4, 9, 12}; DVGO_ERANGE otherwise.
 * --------------------------------------------------------------------------------- */
int dvgo_n_bricks(int X, int Y, int Z);
int dvgo_brick_slice(void);     /* default slice_len: entries per work item of dvgo_brick_accumulate (heavy bricks are cut
                                 * into slices); the scan and the accumulation of one step must be given the same value (>= 256) */
/* counts [n] -> offsets [n+1] + fill cursors [n].  With extra_off / active [n+1] and extra_brick (all or none; then
 * n < 2^18 and the total must stay below 2^28 entries) also the work tables of dvgo_brick_accumulate:
 *   - a brick with more than slice_len entries runs as ceil(count / slice_len) work items -- its own plus EXTRA ones
 *     appended behind the bricks (extra_off[n] = their number <= E / slice_len, extra_brick[x] = the brick of extra item x);
 *   - active[0 .. active[n]) = the non-empty bricks in brick order;
 *   - brick_cnt is CLEARED: it becomes the arrival counter array of the slices. */
int dvgo_brick_scan(int32_t* brick_cnt, int n_bricks, int32_t* brick_off, int32_t* brick_cursor, int32_t* extra_off,
                    int32_t* active, int32_t* extra_brick /* [n_extra_max] */, int n_extra_max, int slice_len, void* stream);
/* the ray scan (n3 [n_rays] -> off3 [n_rays + 1], int64) and dvgo_brick_scan in one launch; brick_cnt == NULL: rays only.
 * With bricks, off3 must have n_rays + 2 entries: off3[n_rays + 1] = brick_off[n_bricks], the total list length, so that the
 * caller's one host read (sample total, list total) is 16 contiguous bytes. */
int dvgo_march_scans(const int32_t* n3, int64_t n_rays, int64_t* off3, int32_t* brick_cnt, int n_bricks,
                     int32_t* brick_off, int32_t* brick_cursor, int32_t* extra_off, int32_t* active, int32_t* extra_brick,
                     int n_extra_max, int slice_len, void* stream);
/* extra_off == NULL: one workgroup per brick, whatever its list length.  Else the work tables of dvgo_brick_scan,
 * `arrive` = the cleared counters, `scratch` = 2 * n_extra_max tiles of 512 * round_up(C + 1, 4) floats, n_extra_max = a
 * host-side upper bound of extra_off[n] (the launch is ceil8(n_bricks) + n_extra_max workgroups). */
int dvgo_brick_accumulate(const int32_t* brick_off, const int32_t* extra_off, const int32_t* active,
                          const int32_t* extra_brick, int32_t* arrive, float* scratch, int64_t n_extra_max, int slice_len,
                          const void* recs, const float* rays_start, const float* rays_dir,
                          float stepdist, const float* xyz_min, const float* xyz_max, const float* grad_feat,
                          int C, int X, int Y, int Z, float* grad_k0, float* grad_density,
                          float* p_k0, float* m_k0, float* v_k0, float step_size_k0, int masked_k0,
                          float* p_density, float* m_density, float* v_density, float step_size_density,
                          int masked_density, float beta1, float beta2, float eps,
                          const float* step_sizes_dev /* NULL, or device {step_size_k0, step_size_density}: read instead of
                                                         the two float arguments (a captured step replays with new values) */,
                          float* tiles, int tiles_mode
                                      /* data parallel (ray-sharded ranks, replicated grids): the gradient travels as whole brick
                                         tiles of 512 x round_up(C + 1, 4) floats, one per brick of `active` = the bricks ANY rank
                                         touched (active[n_bricks] = their number; from dvgo_brick_scan over the all-reduced
                                         counts).  tiles_mode 2: accumulate this rank's lists and write tiles[i] for every
                                         brick active[i] (zeros where this rank has no entry); the caller all-reduces `tiles`;
                                         tiles_mode 3: read tiles[i] and apply the (masked) Adam update of brick active[i] from
                                         it (lists / recs / rays unused).  0: neither. */,
                          void* stream);

/* Combined gradient rows G [n_vox][row_stride] (built by the two calls above) -> the channels-last feature
 * gradient [n_vox][C] and the density gradient [n_vox], both fully written.  Built for row_stride 16, C 12. */
int dvgo_grid_grad_split(const float* G, int64_t n_vox, int row_stride, int C, float* grad_k0, float* grad_density,
                         void* stream);

/* ---------------------------------------------------------------------------------
 * "next" row N4: coarse-stage grid maintenance.
 *   voxel_count_views (lib/dvgo.py:265-295): per training view, acc[v] = sum of the trilinear weights voxel v receives
 *   from the view's sample points (o + d * (t_min + k * step / |d|), k < n_samples, t_min = slab entry clamped to
 *   [near, far]); count[v] += (acc[v] > 1).  Call dvgo_view_weight_accumulate for the rays of ONE view (any number of
 *   calls), then dvgo_view_count_commit, which also clears acc for the next view.  acc, count: [X*Y*Z] floats, acc zero
 *   on first use.  xyz_min / xyz_max are HOST pointers.
 *   maskout_near_cam_vox (lib/dvgo.py:215-226): density[v] = value where min_c |xyz(v) - cam_o[c]| <= near;
 *   grid_x/y/z are the per-axis voxel-centre coordinates (device, [X] / [Y] / [Z]), cam_o [n_cam,3].
 * --------------------------------------------------------------------------------- */
int dvgo_view_weight_accumulate(const float* rays_o, const float* rays_d, int64_t n_rays, const float* xyz_min,
                                const float* xyz_max, float near, float far, float step, int n_samples, int X, int Y,
                                int Z, float* acc, void* stream);
int dvgo_view_count_commit(float* acc, float* count, int64_t n_vox, void* stream);
/* dvgo_rays_of_view: rays of the pixels [p0, p0 + n) (row-major) of one view -- lib/ray_utils.py:9-85: get_rays (pixel
 *   coordinates, `center` = mode 'center' else 'lefttop', flips, inverse_y), viewdirs = rays_d / |rays_d| (before the NDC
 *   warp, as get_rays_of_a_view), ndc != 0: ndc_rays(H, W, ndc_focal, ndc_near, ...).  K4 = {fx, fy, cx, cy} and c2w (3 x 4,
 *   row-major) are HOST pointers; outputs [n, 3] device arrays (viewdirs may be NULL). */
int dvgo_rays_of_view(int H, int W, const float* K4, const float* c2w, int inverse_y, int flip_x, int flip_y, int center,
                      int ndc, float ndc_focal, float ndc_near, int64_t p0, int64_t n,
                      float* rays_o, float* rays_d, float* viewdirs, void* stream);
int dvgo_maskout_near_cam(float* density, const float* grid_x, const float* grid_y, const float* grid_z, int X, int Y, int Z,
                          const float* cam_o, int n_cam, float near, float value, void* stream);

/* ---------------------------------------------------------------------------------
 * "next" row N3: fused colour head (rgbnet) forward.  Replaces lib/dvgo.py:516-541 for the
 * Sequential(Linear(d_in,width), ReLU, Linear(width,width), ReLU, Linear(width,3)) head:
 *   x   = cat([feat[:, 3:] if diffuse else feat, emb[ray_id]])       d_in = C - (3 if diffuse) + E
 *   rgb = sigmoid(MLP(x) + (feat[:, :3] if diffuse))
 * feat [M,C], emb [N_rays,E] (view-direction embedding per ray), ray_id [M] int64.  Weights in
 * nn.Linear layout ([out,in] row-major).  fp32 throughout (v_mfma_f32_32x32x2_f32).
 * Training (all or none): H1, H2 [M,width] = post-ReLU activations, row-major (operands of the weight
 * gradients), and masks [M][2 layers][2 lane halves] uint64 = their sign bits in accumulator order (the ReLU
 * masks of dvgo_shade_bwd: 32 B per sample instead of re-reading 1 KB of activations).
 * Returns DVGO_ERANGE for shapes outside the built set (width == 128, d_in <= 40): fall back.
 * --------------------------------------------------------------------------------- */
int dvgo_shade_fwd(const float* feat, int C, const float* emb, int E, const int64_t* ray_id, int64_t M, const int64_t* m_dev,
                   const float* W1, const float* b1, const float* W2, const float* b2,
                   const float* W3, const float* b3, int width, int d_in, int diffuse,
                   float* rgb, float* H1, float* H2, uint64_t* masks,
                   void* scratch /* NULL, or dvgo_shade_scratch_bytes(width) bytes of device memory */,
                   void* scratch_bwd /* NULL, or a second block of that size: a training step has the weight image of the
                                        data-gradient kernel built by the same prep launch (dvgo_shade_bwd: prebuilt = 1) */,
                   void* stream);

/* Kernel variants of the colour head (process-global, for A/B runs; returns the previous value, negative = query):
 *   bit 0  forward, bit 1 data gradients on the bf16 matrix cores: every fp32 operand split EXACTLY into three bf16
 *          pieces, six partial products per k-step accumulated in fp32 (csrc/shade_x3.hip) -- fp32-grade results at 2.7x
 *          fewer matrix-pipe cycles than v_mfma_f32_32x32x2_f32.  The f32-MFMA kernels run when the bit is
 *          clear or `scratch` is NULL (the bf16 variants keep the pre-split weight image there, built by a small kernel
 *          at every call).
 *   weight gradients (dvgo_shade_wgrad), first match wins:
 *     bit 5 (32)  two barrier-free kernels on the split operands, every operand straight from global memory (shade_x3.hip c1/c2)
 *     bit 2 (4)   split operands staged through LDS, one 8-wave workgroup per CU; + bit 4 (16): 4-wave workgroups, two per CU
 *     bit 6 (64)  the pipelined LDS-DMA ring with the contraction on the split operands, B fragments shared through LDS
 *     none        the pipelined LDS-DMA ring with v_mfma_f32_32x32x2_f32 (bit 3 (8): the round-1 kernel instead)
 *   Default 67 = 1 | 2 | 64 (measured, roofline case: weight gradients 0.93 -> 0.72 ms against the f32 ring). */
int64_t dvgo_shade_scratch_bytes(int width);
int dvgo_shade_variant(int flags);

/* Data-gradient part of the colour-head backward.  Inputs: g_rgb, rgb [M,3]; the saved activations
 * sign-bit masks written by dvgo_shade_fwd.  Outputs: gz [M,3] (= g_rgb * sigmoid'),
 * G1 = relu'(H1) * (W2^T G2) as [M,width] where G2 = relu'(H2) * (W3^T gz) stays in registers (dvgo_shade_wgrad
 * rebuilds it from gz and the masks rather than streaming 512 B/sample), and g_feat [M,C] fully written:
 * channels [0,3) = gz when diffuse, channels [c0, C) = (W1^T G1)[:C-c0]. */
int dvgo_shade_bwd(const float* g_rgb, const float* rgb, const uint64_t* masks, int64_t M, const int64_t* m_dev,
                   const float* W1, const float* W2, const float* W3, int width, int d_in, int C, int diffuse,
                   float* g_feat, float* G1, float* gz, void* scratch,
                   int prebuilt /* scratch already holds this kernel's weight image (dvgo_shade_fwd: scratch_bwd) */,
                   void* stream);

/* Weight-gradient part (G1, gz from dvgo_shade_bwd; masks, H1, H2 from dvgo_shade_fwd; W3 as given to both):
 * dW2 = G2^T H1, dW1 = G1^T X (X = the layer-1 input, re-assembled from feat / emb /
 * ray_id exactly as in dvgo_shade_fwd), dW3 = gz^T H2 and the three bias gradients (column sums); fp32 MFMA
 * with both operands read row-major straight from memory.  Every one of the n_parts workgroups writes its
 * partial sums to part[p] = { dW2 [width][width], dW1 [width][64], dW3 [32][width] (rows 0..2 valid),
 * db1 [width], db2 [width], db3 [width] (db3[c] = entry c + entry 8+c, c < 3) } floats (scratch), and a second launch sums them over p
 * into `total`, the compact record { dW2 [width][width], dW1 [width][d_in], dW3 [3][width], db1 [width], db2 [width], db3 [3] }
 * (d_in = (C - 3 * diffuse) + E; width^2 + width * d_in + 5 * width + 3 floats): views of it are the gradients. */
int dvgo_shade_wgrad(const float* G1, const float* gz, const uint64_t* masks, const float* W3,
                     const float* H1, const float* H2, const float* feat, int C, const float* emb, int E, const int64_t* ray_id, int64_t M,
                     const int64_t* m_dev, int width, int diffuse, int n_parts, float* part, float* total, void* stream);

/* ---------------------------------------------------------------------------------
 * Positional-encoding colour head (posbase_pe = P > 0, lib/dvgo.py:528-534), csrc/shade_pe.hip:
 *   X   = cat([pts, sin(pts (x) freq), cos(pts (x) freq), emb[ray_id]])    d_in = 3 + 6P + E columns, never stored
 *   rgb = sigmoid(W3 relu(W2 relu(W1 X + b1) + b2) + b3)                     no diffuse term; the feature grid is unused
 * Built for width 128 and d_in <= 96 (P <= 10 with the view embedding of viewbase_pe = 4); DVGO_ERANGE otherwise: fall
 * back.  freq [P] is the model's posfreq buffer (2^j), emb [n_rays, E] the output of dvgo_viewdir_embed.
 * dvgo_march_positions: pts [M,3] = start + dir * stepdist * step_id of the fused march's kept samples (the expression
 *   of dvgo_sample_pts_on_rays, so the positions equal its ray_pts bit for bit).
 * dvgo_shade_pe_fwd: rgb [M,3]; H1, H2 [M,width] and masks [M,4] (ReLU sign bits, as dvgo_shade_fwd) all NULL, or all
 *   given (training).
 * dvgo_shade_pe_bwd: gz [M,3] = g_rgb * sigmoid', G1 [M,width] = relu'(H1) * (W2^T (relu'(H2) * (W3^T gz))).
 *   Positions and view directions carry no gradient: there is no input gradient.
 * dvgo_shade_pe_wgrad: n_parts workgroups write partial records (part: n_parts * dvgo_shade_pe_record_size floats) and a
 *   second launch sums them into `total`, the compact record of dvgo_shade_wgrad
 *   { dW2 [width][width], dW1 [width][d_in], dW3 [3][width], db1 [width], db2 [width], db3 [3] }; X is rebuilt from
 *   pts, freq, emb and ray_id exactly as in the forward.
 * M == 0 (a batch in which no sample survives) is valid for all three: arguments that do not depend on M are checked
 *   as usual, then the call returns 0 without a launch and without looking at the array pointers, which may be NULL
 *   (an empty tensor has no storage).  dvgo_shade_pe_fwd and dvgo_shade_pe_bwd write nothing; dvgo_shade_pe_wgrad
 *   zeroes `total` (required), so the gradients of an empty batch are zeros, and leaves `part` alone. */
int dvgo_march_positions(const float* rays_start, const float* rays_dir, const int64_t* ray_id, const int64_t* step_id,
                         int64_t M, float stepdist, float* pts, void* stream);
int dvgo_shade_pe_fwd(const float* pts, const float* freq, int P, const float* emb, int E, const int64_t* ray_id, int64_t M,
                      const float* W1, const float* b1, const float* W2, const float* b2, const float* W3, const float* b3,
                      int width, int d_in, float* rgb, float* H1, float* H2, uint64_t* masks, void* stream);
int dvgo_shade_pe_bwd(const float* g_rgb, const float* rgb, const uint64_t* masks, int64_t M, const float* W2,
                      const float* W3, int width, float* G1, float* gz, void* stream);
int64_t dvgo_shade_pe_record_size(int width, int d_in);
int dvgo_shade_pe_wgrad(const float* G1, const float* gz, const uint64_t* masks, const float* W3, const float* H1,
                        const float* H2, const float* pts, const float* freq, int P, const float* emb, int E,
                        const int64_t* ray_id, int64_t M, int width, int d_in, int n_parts, float* part, float* total,
                        void* stream);

/* ---------------------------------------------------------------------------------
 * "next" rows N1/N2: optimizer and regulariser kernels.
 *   adam_upd_cuda.{adam_upd,masked_adam_upd,adam_upd_with_perlr}
 *     (lib/cuda/adam_upd.cpp:36-86, adam_upd_kernel.cu) -- mode 0/1/2, in place.
 *     step_size is computed by the caller exactly as the reference host code does (:72).
 *   total_variation_cuda.total_variation_add_grad
 *     (lib/cuda/total_variation.cpp:16-24, total_variation_kernel.cu) -- in place on grad.
 * --------------------------------------------------------------------------------- */
int dvgo_adam_upd(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                  const float* perlr /* mode 2 only */, int64_t n, float step_size,
                  float beta1, float beta2, float eps, int mode, void* stream);

/* Adam / masked Adam (mode 0 / 1, as dvgo_adam_upd) for the feature grid (channels-last rows [n_vox][C]) and the
 * density grid [n_vox] straight from the combined gradient rows G [n_vox][row_stride] of dvgo_march_feat_bwd /
 * dvgo_march_density_bwd -- instead of dvgo_grid_grad_split followed by two dvgo_adam_upd.  Built for row_stride 16,
 * C 12.  step_size_* as for dvgo_adam_upd (computed by the caller in float, adam_upd_kernel.cu:72). */
int dvgo_adam_rows(const float* G, int64_t n_vox, int row_stride, int C,
                   float* p_k0, float* m_k0, float* v_k0, float step_size_k0, int mode_k0,
                   float* p_density, float* m_density, float* v_density, float step_size_density, int mode_density,
                   float beta1, float beta2, float eps, void* stream);

int dvgo_total_variation_add_grad(const float* param, float* grad, float wx, float wy, float wz,
                                  int64_t C, int64_t sz_i, int64_t sz_j, int64_t sz_k,
                                  int64_t sC, int64_t sI, int64_t sJ, int64_t sK,
                                  int dense_mode, void* stream);
/* The same, restricted to the planes [i_lo, i_hi) of the first spatial axis (only their `grad` is touched; `param` is
 * read one plane beyond on either side).  For a data-parallel rank that owns one slab of the grid.  Needs a layout whose
 * outermost memory axis is that spatial axis (channels-last, or C == 1), else DVGO_ERANGE. */
int dvgo_total_variation_add_grad_slab(const float* param, float* grad, float wx, float wy, float wz,
                                       int64_t C, int64_t sz_i, int64_t sz_j, int64_t sz_k, int64_t sC,
                                       int64_t sI, int64_t sJ, int64_t sK, int dense_mode, int64_t i_lo, int64_t i_hi,
                                       void* stream);

/* ---------------------------------------------------------------------------------
 * Harness glue (row H3): fused training loss, view-direction embedding, multi-tensor Adam.
 *
 * dvgo_loss_fwd_bwd: the loss of run.py:377-386 and its gradients in one pass.
 *   loss = w_main * sum((rgb_marched - target)^2) / (3 n_rays_global)
 *        + w_ent  * sum(-(p log p + (1-p) log(1-p))) / n_rays_global,  p = clamp(alphainv_last, 1e-6, 1-1e-6)
 *        + w_per  * sum_i weights_i * |raw_rgb_i - target[ray_id_i]|^2 / n_rays_global   (weights detached)
 *   Writes loss_out[0] (device scalar) and d loss / d {rgb_marched [N,3], alphainv_last [N], raw_rgb [M,3]}.
 *   n_rays_global is the ray count over all ranks (data parallel).
 * dvgo_viewdir_embed: emb [N, 3 + 6F] = cat([v, sin(v (x) freq), cos(v (x) freq)]) (lib/dvgo.py:524-525).
 * dvgo_adam_upd_multi: plain Adam (mode 0 of dvgo_adam_upd) over up to 16 small tensors in one launch;
 *   the pointer tables and numel are HOST arrays.  A tensor with numel[k] == 0 is skipped and its four pointers may be
 *   NULL (an empty torch tensor has no memory), as in dvgo_copy_multi; a NULL pointer with numel[k] > 0 is DVGO_EINVAL.
 * --------------------------------------------------------------------------------- */
int dvgo_loss_fwd_bwd(const float* rgb_marched, const float* alphainv_last, const float* target, int64_t N,
                      const float* raw_rgb, const float* weights, const int64_t* ray_id, int64_t M, const int64_t* m_dev,
                      int64_t n_rays_global, float w_main, float w_ent, float w_per,
                      float* g_marched, float* g_last, float* g_raw_rgb, float* loss_out, void* stream);
/* dvgo_copy_multi: dst[k][0 .. n_dwords[k]) = src[k][...] for up to 8 (dst, src) pairs of 4-byte elements in ONE launch
 * (harness plumbing: the batch of a captured training step is copied into the graph's input tensors). */
int dvgo_copy_multi(void* const* dst, const void* const* src, const int64_t* n_dwords, int n_tensors, void* stream);
int dvgo_viewdir_embed(const float* viewdirs, const float* freq, int n_freq, int64_t N, float* emb, void* stream);
int dvgo_adam_upd_multi(float* const* params, const float* const* grads, float* const* exp_avg,
                        float* const* exp_avg_sq, const int64_t* numel, int n_tensors, float step_size,
                        float beta1, float beta2, float eps,
                        const float* step_size_dev /* NULL, or the step size on the device */, void* stream);

/* ---------------------------------------------------------------------------------
 * Image metrics of rendered views.  lib/utils.py:88-134 (rgb_ssim) / run.py:116-121
 * img0, img1 [n,H,W,3] fp32, contiguous: n same-sized pairs (one call per view size).
 *   ssim_sum[n] (double): the sum of the SSIM map of each pair over its (H-fs+1) x (W-fs+1) x 3 entries;
 *                         SSIM = ssim_sum / that count.
 *   sse[n]      (double): sum over all H*W*3 values of (img0 - img1)^2 (the difference squared in fp32, as run.py:117
 *                         forms it); PSNR = -10 log10(sse / (H*W*3)).
 *   ssim_map: NULL, or [n, H-fs+1, W-fs+1, 3] fp32.
 *   taps: HOST array of the filter_size Gaussian taps, computed in float64 as lib/utils.py:101-105 does;
 *   c1 = (k1 max_val)^2, c2 = (k2 max_val)^2.
 *   workspace: DEVICE scratch of at least dvgo_image_metrics_workspace_bytes(n, H, W, filter_size) bytes.
 * The x^2, y^2, xy products are rounded to fp32 as the reference forms them; blurs, map and sums are fp64.  Results are
 * bitwise reproducible and the same for an image whether it is scored alone or at any place in a batch.
 * DVGO_EINVAL: H or W < filter_size (the reference's empty mean, nan), non-positive sizes, null pointers, a short
 * workspace.  DVGO_ERANGE: filter_size > 16, H*W*3 >= 2^31, or more than 2^31 tiles.  n == 0 is a no-op.
 * dvgo_image_metrics_workspace_bytes returns the byte count, or the error code for the sizes.
 * --------------------------------------------------------------------------------- */
int64_t dvgo_image_metrics_workspace_bytes(int64_t n, int H, int W, int filter_size);
int dvgo_image_metrics(const float* img0, const float* img1, int64_t n, int H, int W, const double* taps, int filter_size,
                       double c1, double c2, double* ssim_sum, double* sse, float* ssim_map,
                       void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * Geometry export: a triangle mesh of the density level set.  Extends the reference's debug exports (run.py:514-553:
 * --export_coarse_only / --export_fine_only dense volumes; tools/vis_volume.py: thresholded voxel cloud) to a closed
 * surface, by marching tetrahedra on the Freudenthal split of an extraction lattice (csrc/mesh.hip).
 *
 * The lattice has Rx x Ry x Rz points, padded by one empty point per side: P = R + 2 per axis, at most 2^28 points
 * (padding included; DVGO_ERANGE above).  A point is inside when its field value > iso.
 * dvgo_mesh_field: field [Px, Py, Pz] fp32 of the padded lattice.  Unpadded point (i, j, k) holds
 *     copy != 0: density[i, j, k] (requires R == (X, Y, Z))
 *     copy == 0: the trilinear sample of density [X, Y, Z] (X, Y, Z >= 2) at grid-index coordinates g = g0 + i * gs
 *                per axis (the corner weights of grid_sample_fwd, zero outside the grid)
 *   unless mask (NULL: all occupied) [MX, MY, MZ] says 0 at the world point box_min + i * spacing, looked up as
 *   maskcache_lookup does (round(fma(xyz, mask_scale, mask_shift)), out of range = 0).  Padding and masked-out
 *   points hold iso - 1.  g0, gs, box_min, spacing, mask_scale, mask_shift: HOST arrays of 3.
 * dvgo_mesh_count: edge_mask [Px*Py*Pz] (uint8: bit d set when the edge to the neighbour in direction
 *   x, y, z, xy, xz, yz, xyz crosses the surface), partials [2 * ceil(Px*Py*Pz / 256)], bases [2 * (that + 1)]
 *   (uint32); bases ends with the totals (V, F): the caller reads those 8 bytes to size the outputs.
 * dvgo_mesh_emit: verts [V, 3] and normals [V, 3] fp32 (world coordinates box_min + i * spacing per axis; unit
 *   normals pointing to lower field values), faces [F, 3] int32 wound outward, in the order DESIGN.md 6c defines.
 *   n_verts / n_faces: the V and F of dvgo_mesh_count (writes past them are dropped).
 * No atomics: the outputs are a function of the field alone.
 * --------------------------------------------------------------------------------- */
int dvgo_mesh_field(const float* density, int X, int Y, int Z, const uint8_t* mask, int MX, int MY, int MZ,
                    const float* mask_scale, const float* mask_shift, int Rx, int Ry, int Rz, const float* g0,
                    const float* gs, const float* box_min, const float* spacing, int copy, float iso, float* field,
                    void* stream);
int dvgo_mesh_count(const float* field, int Px, int Py, int Pz, float iso, uint8_t* edge_mask, uint32_t* partials,
                    uint32_t* bases, void* stream);
int dvgo_mesh_emit(const float* field, const uint8_t* edge_mask, const uint32_t* bases, int Px, int Py, int Pz,
                   float iso, const float* box_min, const float* spacing, int64_t n_verts, int64_t n_faces,
                   float* verts, float* normals, int32_t* faces, void* stream);

/* ---------------------------------------------------------------------------------
 * Unbounded scenes (csrc/contract.hip).  Per ray, in float32:
 *   o' = (o - center) / radius, u = d / radius, d' = u / ||u||_2, p_k = o' + d' * t_tab[k] (k < n_max),
 *   n_k = max|p_k| (l2 == 0) or ||p_k||_2 (l2 != 0), q_k = p_k if n_k <= 1 else p_k / n_k * ((1 + b) - b / n_k),
 *   kept when (n_k <= 1 or acc > thres after acc += ||q_k - q_{k-1}||_2, acc reset to 0 on keep) and the
 *   occupancy mask [mi, mj, mk] (NULL: all occupied) holds at q_k (maskcache_lookup's rounding).
 * dvgo_contract_count: counts [n_rays] int32 = kept samples per ray.
 * dvgo_contract_emit:  offsets [n_rays + 1] = dvgo_exclusive_scan_i32(counts); writes the kept samples ray-major,
 *   step-ascending: q [M, 3], ray_id [M], step_id [M] (= k), t [M] (= t_tab[k]).
 * center, radius: device float[3].  thres = (2 + 2b) / W * stepsize * 0.95.
 * dvgo_distortion_fwd_bwd: w, s [m] of ray-sorted samples (ray_id [m] in [0, n_rays)), delta = 1 / n_max,
 *   loss = (1/n_norm) sum_rays [2 sum_i w_i (s_i W_<i - S_<i) + delta/3 sum_i w_i^2], grad [m] = dloss/dw.
 *   partials: double [ceil(n_rays / 256)] scratch; ticket: one uint32 that must be 0 on entry.
 *   Deterministic: fixed-order reductions, no float atomics.
 * --------------------------------------------------------------------------------- */
int dvgo_contract_count(const float* rays_o, const float* rays_d, int64_t n_rays, const float* center,
                        const float* radius, const float* t_tab, int n_max, float bg_len, int l2, float thres,
                        const uint8_t* mask, int mi, int mj, int mk, const float* mask_scale,
                        const float* mask_shift, int32_t* counts, void* stream);
int dvgo_contract_emit(const float* rays_o, const float* rays_d, int64_t n_rays, const float* center,
                       const float* radius, const float* t_tab, int n_max, float bg_len, int l2, float thres,
                       const uint8_t* mask, int mi, int mj, int mk, const float* mask_scale, const float* mask_shift,
                       const int64_t* offsets, float* q, int64_t* ray_id, int64_t* step_id, float* t,
                       void* stream);
int dvgo_distortion_fwd_bwd(const float* w, const float* s, const int64_t* ray_id, int64_t m, int64_t n_rays,
                            int64_t n_norm, int n_max, float* grad, double* partials, unsigned int* ticket,
                            float* loss, void* stream);

/* ---------------------------------------------------------------------------------
 * Tri-plane features (csrc/triplane.hip).  Replaces lib/tri_dvgo.py:456-469 grid_sampler2D:
 * three F.grid_sample(plane[1,C,H,W], ind_norm[..., pair], mode='bilinear', align_corners=True) calls, the
 * transposes, and torch.cat (sum == 0) or xy + yz + zx (sum != 0), and their autograd backward w.r.t. the planes.
 * Planes xy, yz, zx: fp32, C channels each, sizes H_s x W_s independent of each other, addressed through ELEMENT
 * strides (sC, sH, sW): channel-first (sW == 1) and channels-last (sC == 1) both work.  The reference's ind_norm is
 * the FLIPPED coordinate triple and grid_sample's first grid component addresses W, so whatever the names suggest:
 *     plane   rows (H) follow world axis   columns (W) follow world axis
 *     xy      y (1)                        z (2)
 *     yz      x (0)                        y (1)
 *     zx      z (2)                        x (0)
 * Per axis g = ((((p - min) / (max - min)) * 2 - 1) + 1) / 2 * (size - 1), f = floor(g), weights (f + 1) - g and
 * g - f; a corner's weight is wh * ww; corners in the order (h0,w0), (h0,w1), (h1,w0), (h1,w1), acc = fmaf(v, w, acc)
 * from 0; corners outside the plane are skipped (zero padding).  A plane axis of size 1 is legal.
 * dvgo_triplane_fwd: xyz [M,3] world coordinates, xyz_min / xyz_max device float[3] -> out [M, 3C] (xy, yz, zx) or,
 *   sum != 0, [M, C] = (xy + yz) + zx.
 * dvgo_triplane_bwd: grad_out as `out`; g_s[c, ih, iw] += w * grad_out[m, c'] (c' = s * C + c, or c when sum != 0)
 *   into the caller's buffers (zero-filled or holding a partial sum; strides as the planes') with float atomics:
 *   the summation order is not reproducible.  No gradient for xyz.  run: consecutive samples one lane sums in
 *   registers while they stay in one texel cell, before its atomics (1: none; 0: the library's default).
 * M == 0 or C == 0: no-op.  DVGO_EINVAL: negative M or C or run, a plane axis < 1, null pointers.  DVGO_ERANGE:
 * M * 3C >= 2^31.
 * --------------------------------------------------------------------------------- */
int dvgo_triplane_fwd(const float* xy, int H_xy, int W_xy, int64_t sC_xy, int64_t sH_xy, int64_t sW_xy,
                      const float* yz, int H_yz, int W_yz, int64_t sC_yz, int64_t sH_yz, int64_t sW_yz,
                      const float* zx, int H_zx, int W_zx, int64_t sC_zx, int64_t sH_zx, int64_t sW_zx,
                      int C, const float* xyz, const float* xyz_min, const float* xyz_max, int64_t M, int sum,
                      float* out, void* stream);
int dvgo_triplane_bwd(const float* grad_out,
                      float* g_xy, int H_xy, int W_xy, int64_t sC_xy, int64_t sH_xy, int64_t sW_xy,
                      float* g_yz, int H_yz, int W_yz, int64_t sC_yz, int64_t sH_yz, int64_t sW_yz,
                      float* g_zx, int H_zx, int W_zx, int64_t sC_zx, int64_t sH_zx, int64_t sW_zx,
                      int C, const float* xyz, const float* xyz_min, const float* xyz_max, int64_t M, int sum,
                      int run, void* stream);

/* ---------------------------------------------------------------------------------
 * Position gradient of the trilinear sample (csrc/grid_sample_xyz.hip): the other half of
 * grid_sampler_3d_backward, d out / d xyz, which the reference never asks for (its poses are constants).  What
 * camera-pose refinement (directvoxgo_amd/pose.py) differentiates through.
 * grid, strides, xyz, xyz_min / xyz_max as dvgo_grid_sample_fwd; grad_out [M,C] row-major; grad_xyz [M,3].
 * Per sample: the cell, the per-axis float32 weights and the in-range test of the gather (floorf chooses the cell: on a
 * lattice plane the derivative is the upper cell's, as in F.grid_sample's backward).  Per channel c, ascending, over the
 * gather's corner order n = 0..7 (bit2 = +X, bit1 = +Y, bit0 = +Z), corners outside the grid skipped (zero padding),
 * each chain from 0:
 *     dX_c = fmaf(v, sx(n) * (wz * wy), dX_c)   dY_c = fmaf(v, sy(n) * (wz * wx), dY_c)   dZ_c = fmaf(v, sz(n) * (wy * wx), dZ_c)
 * with the sign -1 on the lower corner of that axis and +1 on the upper; then ax = fmaf(grad_out[m,c], dX_c, ax), and
 * grad_xyz[m,0] = ax * ((float)(X-1) / (xyz_max[0] - xyz_min[0])); likewise y and z.  A sample whose eight corners
 * are all outside gets 0.0f, an axis of size 1 gives 0 on that axis.  Every row is written with plain stores by one
 * lane: no atomics, no workspace, and grad_xyz need not be zeroed.  Channels-last with C % 4 == 0 and 16-byte aligned
 * grid and grad_out reads 16-byte vectors; everything else goes through the element strides.
 * M == 0: no-op.  DVGO_EINVAL: negative M or C, an axis < 1, null pointers with M > 0.  DVGO_ERANGE: M * C >= 2^31.
 * --------------------------------------------------------------------------------- */
int dvgo_grid_sample_bwd_xyz(const float* grid, int C, int X, int Y, int Z,
                             int64_t sC, int64_t sX, int64_t sY, int64_t sZ,
                             const float* grad_out, const float* xyz, const float* xyz_min, const float* xyz_max,
                             int64_t M, float* grad_xyz, void* stream);

/* ---------------------------------------------------------------------------------
 * LIIF plane decoder around its MLPs (csrc/liif.hip).  Replaces lib/tri_dvgo.py:481-565
 * liif_interpolate except the Interp_MLP calls: per sample, plane and shifted position the nearest texel's features, the
 * relative coordinates and the cell sizes as one MLP input row, the blend weights, the blend, and both gradients.
 * Planes as in dvgo_triplane_*: pointer, H, W and three ELEMENT strides each, any dense layout.  (Wx, Wy, Wz) = world_size.
 * All of the following in float32, in this order, no contraction:
 *   n_a = ((p_a - min_a) / (max_a - min_a)) * 2 - 1                      for world axis a
 *     plane   u (addresses rows, H_s)   v (addresses columns, W_s)   (Ta, Tb)
 *     xy      n_z                       n_y                          (Wx, Wy)
 *     yz      n_y                       n_x                          (Wy, Wz)
 *     zx      n_x                       n_z                          (Wz, Wx)
 *   shifts e = 0..3: (vx, vy) = (-1,-1), (-1,+1), (+1,-1), (+1,+1); E = 4.  local_ensemble == 0: one shift, E = 1,
 *     with u' = clamp(u), v' = clamp(v).
 *   u' = clamp(u + (vx * (1 / Ta) + 1e-6f), (float)(-1 + 1e-6), (float)(1 - 1e-6));   v' likewise with vy, 1 / Tb
 *   near_S(c) = clip(rint(((c + 1) * S - 1) / 2), 0, S - 1), rint to even (grid_sample 'nearest', align_corners=False)
 *   texel: row near_H(u'), column near_W(v')
 *   q0 = node_Tb(near_Tb(v')), q1 = node_Ta(near_Ta(u')), node_T(i) = i * (2 / (T - 1)) - 1, node_1 = -1
 *   rel0 = (u - q0) * H_s, rel1 = (v - q1) * W_s        (u against the v table: the reference's pairing)
 *   row of inp: plane[:, row, col] (C values), rel0, rel1, then, cell_decode != 0, (1 / Ta) * H_s, (1 / Tb) * W_s:
 *     D = C + 2 or C + 4
 *   area_e = |rel0 * rel1| + 1e-9f; tot = ((a0 + a1) + a2) + a3; wgt_e = area_{E-1-e} / tot
 * dvgo_liif_gather: xyz [M,3], xyz_min / xyz_max device float[3] -> inp [3, E, M, D], wgt [3, E, M], dense.  Channels-last
 *   planes with 16-byte (C % 4 == 0 and D % 4 == 0) or 8-byte (C % 2 == 0) aligned texels are read and written in
 *   pieces of that size; everything else goes element by element through the strides.
 * dvgo_liif_scatter: g_s[c, row, col] += grad_inp[s, e, m, c] (the first C columns of each row) into the caller's buffers
 *   (zero-filled or holding a partial sum; strides as the planes') with float atomics: the summation order is not
 *   reproducible.  Texels are recomputed from xyz.  run: consecutive samples a lane sums in a register while they share
 *   a texel (1: none; 0: the library's default, 4: started as a guess, measured since at one batch size only,
 *   profiles/liif/README.md).
 * dvgo_liif_blend_fwd: pred [3, E, M, C], wgt -> out [M, 3C] (sum == 0: xy, yz, zx) or [M, C] (sum != 0: (xy + yz) + zx);
 *   per plane acc = fmaf(pred, wgt, acc) from 0 in shift order.
 * dvgo_liif_blend_bwd: grad_pred[s, e, m, c] = grad_out[m, c'] * wgt[s, e, m] (c' = s * C + c, or c when sum != 0).
 * M == 0 or C == 0: no-op.  DVGO_EINVAL: negative M, C or run, a plane axis or world extent < 1, E not 1 or 4, null
 * pointers.  DVGO_ERANGE: M * 3 E D (gather, scatter) or M * 3 E C (blend) >= 2^31.
 * --------------------------------------------------------------------------------- */
int dvgo_liif_gather(const float* xy, int H_xy, int W_xy, int64_t sC_xy, int64_t sH_xy, int64_t sW_xy,
                     const float* yz, int H_yz, int W_yz, int64_t sC_yz, int64_t sH_yz, int64_t sW_yz,
                     const float* zx, int H_zx, int W_zx, int64_t sC_zx, int64_t sH_zx, int64_t sW_zx,
                     int C, const float* xyz, const float* xyz_min, const float* xyz_max, int64_t M,
                     int Wx, int Wy, int Wz, int cell_decode, int local_ensemble, float* inp, float* wgt, void* stream);
int dvgo_liif_scatter(const float* grad_inp,
                      float* g_xy, int H_xy, int W_xy, int64_t sC_xy, int64_t sH_xy, int64_t sW_xy,
                      float* g_yz, int H_yz, int W_yz, int64_t sC_yz, int64_t sH_yz, int64_t sW_yz,
                      float* g_zx, int H_zx, int W_zx, int64_t sC_zx, int64_t sH_zx, int64_t sW_zx,
                      int C, const float* xyz, const float* xyz_min, const float* xyz_max, int64_t M,
                      int Wx, int Wy, int Wz, int cell_decode, int local_ensemble, int run, void* stream);
int dvgo_liif_blend_fwd(const float* pred, const float* wgt, int C, int64_t M, int E, int sum, float* out, void* stream);
int dvgo_liif_blend_bwd(const float* grad_out, const float* wgt, int C, int64_t M, int E, int sum, float* grad_pred,
                        void* stream);

/* ---------------------------------------------------------------------------------
 * Bilinear plane decoder in front of its MLPs (csrc/plane_rows.hip).  Replaces lib/tri_dvgo.py:568-607
 * interpolate (implicit_voxel_feat=True, liif=False) except the Interp_MLP calls: three F.grid_sample on the planes, three
 * more on two-channel coordinate tables rebuilt per call (make_coord, :311-357), the positional encoding and the cats.
 * Planes as in dvgo_triplane_*: pointer, H, W and three ELEMENT strides each, any dense layout.  (Wx, Wy, Wz) = world_size.
 * All of the following in float32, in this order, no contraction:
 *   ind_norm = (n_z, n_y, n_x), n_a = ((p_a - min_a) / (max_a - min_a)) * 2 - 1, as dvgo_triplane_fwd forms it
 *     plane   c0 (addresses columns)   c1 (addresses rows)   table (Ta rows, Tb columns)   cell
 *     xy      n_z                      n_y                   (Wx, Wy)                      (1 / Wx, 1 / Wy)
 *     yz      n_y                      n_x                   (Wy, Wz)                      (1 / Wy, 1 / Wz)
 *     zx      n_x                      n_z                   (Wz, Wx)                      (1 / Wz, 1 / Wx)
 *   feat (C values): the plane's bilinear sample at (c0, c1), align_corners=True, zero padding: dvgo_triplane_fwd's
 *     per-plane arithmetic, corner order and fma chain, the same bits as its sum == 0 output.
 *   q0, q1: the bilinear sample, by the same rule (g = ((c + 1) / 2) * (T - 1) per axis, weights (f + 1) - g and g - f,
 *     corners (i0,j0), (i0,j1), (i1,j0), (i1,j1), acc = fmaf(v, wi * wj, acc) from 0, corners outside skipped), of a table
 *     [Ta, Tb] that is never built: q0 takes v = node_Tb(j), q1 takes v = node_Ta(i), node_T(i) = i * (2 / (T - 1)) - 1,
 *     node_1 = -1.  The table follows the world lattice of the plane's NAME and is addressed by the flipped coordinates;
 *     its extents are independent of (H_s, W_s).  Inside the box q ~ (c0, c1); all corners outside: q = 0.
 *   encoding: arg = q_k * 2^j, k = 0, 1, j = 0..P-1, k-major (exact); sinf(arg) for all 2P, then cosf(arg) for all 2P.
 *   cell_a = 1.f / Ta, cell_b = 1.f / Tb, with cell_decode != 0.
 *   row = [feat | q0, q1 | sin (2P) | cos (2P) | cell_a, cell_b]: D = C + 2 + 4P (+ 2).
 * dvgo_plane_rows_fwd: xyz [M,3], xyz_min / xyz_max device float[3] -> inp [3, M, D] (xy, yz, zx), dense.  Channels-last
 *   planes with 16-byte (C % 4 == 0 and D % 4 == 0) or 8-byte (C % 2 == 0) aligned texels and an `inp` aligned alike are
 *   read and written in pieces of that size; everything else goes element by element through the strides.
 * dvgo_plane_rows_bwd: g_s[c, ih, iw] += w * grad_inp[s, m, c] for the first C columns of each row (columns >= C are never
 *   read) into the caller's buffers (zero-filled or holding a partial sum; strides as the planes') with float atomics: the
 *   summation order is not reproducible.  No gradient for xyz.  run as in dvgo_triplane_bwd (0: the library's default).
 * M == 0 or C == 0: no-op.  DVGO_EINVAL: negative M, C or run, a plane axis or world extent < 1, P < 1, null pointers.
 * DVGO_ERANGE: 3 M D >= 2^31.
 * --------------------------------------------------------------------------------- */
int dvgo_plane_rows_fwd(const float* xy, int H_xy, int W_xy, int64_t sC_xy, int64_t sH_xy, int64_t sW_xy,
                        const float* yz, int H_yz, int W_yz, int64_t sC_yz, int64_t sH_yz, int64_t sW_yz,
                        const float* zx, int H_zx, int W_zx, int64_t sC_zx, int64_t sH_zx, int64_t sW_zx,
                        int C, const float* xyz, const float* xyz_min, const float* xyz_max, int64_t M,
                        int Wx, int Wy, int Wz, int P, int cell_decode, float* inp, void* stream);
int dvgo_plane_rows_bwd(const float* grad_inp,
                        float* g_xy, int H_xy, int W_xy, int64_t sC_xy, int64_t sH_xy, int64_t sW_xy,
                        float* g_yz, int H_yz, int W_yz, int64_t sC_yz, int64_t sH_yz, int64_t sW_yz,
                        float* g_zx, int H_zx, int W_zx, int64_t sC_zx, int64_t sH_zx, int64_t sW_zx,
                        int C, const float* xyz, const float* xyz_min, const float* xyz_max, int64_t M,
                        int Wx, int Wy, int Wz, int P, int cell_decode, int run, void* stream);

/* ---------------------------------------------------------------------------------
 * Vector-matrix (VM) decomposed features (csrc/vm.hip).  TensoRF's VM
 * decomposition (Chen et al., ECCV 2022): every plane component is multiplied by a 1-D line along the world axis its plane
 * does not see.  No counterpart in the reference; the contract is this text.
 * Planes xy, yz, zx as in dvgo_triplane_*: fp32 [1, R, H_s, W_s], pointer, H, W and three ELEMENT strides each.  Lines
 * l_xy, l_yz, l_zx: fp32 [1, R, N_s, 1], pointer, N and two ELEMENT strides each (lC: component, lN: node).  Any dense layout;
 * every size is independent of the others; a size of 1 on any axis is legal.
 *     plane   rows (H) follow world axis   columns (W) follow world axis   line follows world axis
 *     xy      y (1)                        z (2)                           x (0)
 *     yz      x (0)                        y (1)                           z (2)
 *     zx      z (2)                        x (0)                           y (1)
 * All in float32, no contraction:
 *   p: the plane's bilinear value, dvgo_triplane_fwd's per-plane arithmetic, corner order and fma chain: the same bits as
 *     its sum == 0 output for that plane and component.
 *   l: g = ((((x_a - min_a) / (max_a - min_a)) * 2 - 1) + 1) / 2 * (N_s - 1), f = floor(g), w0 = (f + 1) - g, w1 = g - f,
 *     l = 0; l = fmaf(v[f], w0, l) if 0 <= f < N_s; l = fmaf(v[f + 1], w1, l) if 0 <= f + 1 < N_s.
 *   out[m, s * R + r] = p * l (one multiply), s in the order xy, yz, zx, r fastest: [M, 3R].
 * dvgo_vm_fwd: xyz [M,3] world coordinates, xyz_min / xyz_max device float[3] -> out [M, 3R].  Bitwise repeatable.
 *   R % 4 == 0 with channels-last (component stride 1), 16-byte aligned planes, lines and out: 16-byte loads and stores;
 *   everything else goes element by element through the strides.
 * dvgo_vm_bwd: the values of planes and lines, grad_out [M, 3R], and six gradient buffers g_s / gl_s (zero-filled or holding
 *   a partial sum) with the shape and strides of the tensor each belongs to:
 *     g_s[r, ih, iw] += k_corner * (l * grad_out[m, s * R + r])       k_corner = wh * ww
 *     gl_s[r, n]     += w_node   * (p * grad_out[m, s * R + r])
 *   with float atomics: the summation order is not reproducible.  No gradient for xyz.
 *   run: consecutive samples one lane sums in registers while they stay in one texel cell (for the planes) and in one
 *     line interval (for the lines), before its atomics (1: none; 0: the library's default).
 *   mode 1: every sum goes to global memory; handles every shape.  mode 2: the node sums go through a table [3][N_s][R]
 *     of float adds in LDS, added to gl_s once per workgroup with r fastest, zeros skipped; legal while the table
 *     (N_xy + N_yz + N_zx) * R * 4 bytes is at most 64 KB.  mode 0: the library's choice, mode 2 where it is legal and
 *     mode 1 elsewhere; its default run is 8 (both measured: profiles/vm/README.md).
 * M == 0 or R == 0: no-op, no pointer is looked at.  DVGO_EINVAL: negative M, R or run, a plane axis or line length < 1,
 * a mode outside 0..2, null pointers, an explicit mode 2 whose table exceeds 64 KB.  DVGO_ERANGE: M * 3R >= 2^31.  All of
 * it is answered before any launch.
 * --------------------------------------------------------------------------------- */
int dvgo_vm_fwd(const float* xy, int H_xy, int W_xy, int64_t sC_xy, int64_t sH_xy, int64_t sW_xy,
                const float* yz, int H_yz, int W_yz, int64_t sC_yz, int64_t sH_yz, int64_t sW_yz,
                const float* zx, int H_zx, int W_zx, int64_t sC_zx, int64_t sH_zx, int64_t sW_zx,
                const float* l_xy, int N_xy, int64_t lC_xy, int64_t lN_xy,
                const float* l_yz, int N_yz, int64_t lC_yz, int64_t lN_yz,
                const float* l_zx, int N_zx, int64_t lC_zx, int64_t lN_zx,
                int R, const float* xyz, const float* xyz_min, const float* xyz_max, int64_t M, float* out, void* stream);
int dvgo_vm_bwd(const float* grad_out,
                const float* xy, int H_xy, int W_xy, int64_t sC_xy, int64_t sH_xy, int64_t sW_xy,
                const float* yz, int H_yz, int W_yz, int64_t sC_yz, int64_t sH_yz, int64_t sW_yz,
                const float* zx, int H_zx, int W_zx, int64_t sC_zx, int64_t sH_zx, int64_t sW_zx,
                const float* l_xy, int N_xy, int64_t lC_xy, int64_t lN_xy,
                const float* l_yz, int N_yz, int64_t lC_yz, int64_t lN_yz,
                const float* l_zx, int N_zx, int64_t lC_zx, int64_t lN_zx,
                float* g_xy, float* g_yz, float* g_zx, float* gl_xy, float* gl_yz, float* gl_zx,
                int R, const float* xyz, const float* xyz_min, const float* xyz_max, int64_t M, int run, int mode,
                void* stream);

/* ---------------------------------------------------------------------------------
 * The VM samplers' gradient with respect to the sample POSITION (csrc/vm_xyz.hip; INTEGRATION.md
 * section 7), which dvgo_vm_bwd and dvgo_vm_density_bwd do not give.  Added without a bump of DVGO_ABI_VERSION, as the
 * entries above were.  Planes, lines and the axis table are those of the VM block above.
 * dvgo_vm_bwd_xyz:          grad_out [M, 3R], g_{s,r} = grad_out[m, s * R + r]  (dvgo_vm_fwd's output)
 * dvgo_vm_density_bwd_xyz:  grad_out [M],     g_{s,r} = grad_out[m]             (dvgo_vm_density_fwd's output)
 * Both: the values of planes and lines, xyz [M,3] -> grad_xyz [M,3].  Every row of grad_xyz is written with plain stores:
 * no atomics, no workspace, nothing to zero beforehand.  One lane per sample, everything in the order below whatever the
 * launch shape, the layout and the alignment (bitwise repeatable, the same bits for every layout of the same values).
 * The cell (h0, w0) of plane s, the node n0 of line s and the float32 weights wh0, wh1, ww0, ww1, w0, w1 are the forward's
 * own, bit for bit, so the derivative is that of the cell the forward chose (floor picks the upper cell on a lattice line).
 * The forward zero-pads: a corner or node out of range is dropped and the weights are not clamped; the derivative drops the
 * same corners and nodes, and there is no `inside` predicate.  A position less than one cell outside the box therefore has
 * a non-zero derivative; more than one cell outside on any axis, or with a NaN coordinate, every term is dropped and the
 * row is exactly 0.0 (for finite grad_out).
 * Per sample m, in float32, no contraction but where fmaf is written:
 *   out[0] = out[1] = out[2] = 0.0f
 *   for s = xy, yz, zx, with (ah, aw, al) = (1, 2, 0), (0, 1, 2), (2, 0, 1) the world axes of rows, columns and line:
 *     Ah = Aw = An = 0.0f
 *     for r = 0 .. R - 1 ascending, v_ij the corner (h0 + i, w0 + j) and v0, v1 the nodes n0, n0 + 1 of component r:
 *       p  = the forward's plane value: 0, then fmaf(v_ij, wh_i * ww_j, p) over the corners 00, 01, 10, 11 in range
 *       l  = the forward's line value:  0, then fmaf(v0, w0, l), fmaf(v1, w1, l) over the nodes in range
 *       dh = 0, then fmaf(v_ij, c_ij, dh) over the corners 00, 01, 10, 11 in range, c = (-ww0, -ww1, +ww0, +ww1)
 *       dw = the same with c = (-wh0, +wh0, -wh1, +wh1)
 *       dn = (v1 if n0 + 1 in range else 0.0f) - (v0 if n0 in range else 0.0f)
 *       t = g_{s,r} * l;  Ah = fmaf(t, dh, Ah);  Aw = fmaf(t, dw, Aw)
 *       u = g_{s,r} * p;  An = fmaf(u, dn, An)
 *     the scales once, after the last component (an axis of size 1 has scale 0 and adds exactly 0):
 *       out[ah] = out[ah] + Ah * ((float)(H_s - 1) / (max[ah] - min[ah]))
 *       out[aw] = out[aw] + Aw * ((float)(W_s - 1) / (max[aw] - min[aw]))
 *       out[al] = out[al] + An * ((float)(N_s - 1) / (max[al] - min[al]))
 *   grad_xyz[m] = out: each world axis has received exactly three contributions, in the order s = xy, yz, zx.
 * dvgo_vm_density_bwd_xyz passes over a sample whose grad_out[m] is exactly 0 (either sign): its row is exactly 0.0.
 * R % 4 == 0 with channels-last, 16-byte aligned planes and lines (dvgo_vm_bwd_xyz: grad_out as well): 16-byte loads;
 * everything else element by element through the strides.  The result is the same.
 * M == 0 or R == 0: no-op, no pointer is looked at.  DVGO_EINVAL: negative M or R, a plane axis or line length < 1, null
 * pointers (grad_out and grad_xyz among them).  DVGO_ERANGE: M * 3R >= 2^31.  The conditions and their order are
 * dvgo_vm_fwd's; all of it is answered before any launch.
 * --------------------------------------------------------------------------------- */
int dvgo_vm_bwd_xyz(const float* xy, int H_xy, int W_xy, int64_t sC_xy, int64_t sH_xy, int64_t sW_xy,
                    const float* yz, int H_yz, int W_yz, int64_t sC_yz, int64_t sH_yz, int64_t sW_yz,
                    const float* zx, int H_zx, int W_zx, int64_t sC_zx, int64_t sH_zx, int64_t sW_zx,
                    const float* l_xy, int N_xy, int64_t lC_xy, int64_t lN_xy,
                    const float* l_yz, int N_yz, int64_t lC_yz, int64_t lN_yz,
                    const float* l_zx, int N_zx, int64_t lC_zx, int64_t lN_zx,
                    int R, const float* grad_out, const float* xyz, const float* xyz_min, const float* xyz_max, int64_t M,
                    float* grad_xyz, void* stream);
int dvgo_vm_density_bwd_xyz(const float* xy, int H_xy, int W_xy, int64_t sC_xy, int64_t sH_xy, int64_t sW_xy,
                            const float* yz, int H_yz, int W_yz, int64_t sC_yz, int64_t sH_yz, int64_t sW_yz,
                            const float* zx, int H_zx, int W_zx, int64_t sC_zx, int64_t sH_zx, int64_t sW_zx,
                            const float* l_xy, int N_xy, int64_t lC_xy, int64_t lN_xy,
                            const float* l_yz, int N_yz, int64_t lC_yz, int64_t lN_yz,
                            const float* l_zx, int N_zx, int64_t lC_zx, int64_t lN_zx,
                            int R, const float* grad_out, const float* xyz, const float* xyz_min, const float* xyz_max,
                            int64_t M, float* grad_xyz, void* stream);

/* ---------------------------------------------------------------------------------
 * Vector-matrix (VM) decomposed density (csrc/vm_density.hip): the 3R
 * products of the VM block above summed into one float per sample, with no [M, 3R] buffer anywhere.  Planes, lines, the
 * axis table and the float32 arithmetic of p (plane value) and l (line value) are those of dvgo_vm_fwd, bit for bit.
 * dvgo_vm_density_fwd: out[m] = sum over s in (xy, yz, zx) and r < R of p_{s,r}(m) * l_{s,r}(m), in float32, as ONE fma
 *   chain in a fixed order: acc = 0; for s = xy, yz, zx: for r = 0 .. R - 1: acc = fmaf(p_{s,r}, l_{s,r}, acc); out[m] =
 *   acc.  The order does not depend on the layout or alignment of planes and lines.  Bitwise repeatable.
 * dvgo_vm_density_bwd: dvgo_vm_bwd's contract with grad_out[m, s * R + r] replaced by grad_out[m] ([M]):
 *     g_s[r, ih, iw] += k_corner * (l * grad_out[m])       gl_s[r, n] += w_node * (p * grad_out[m])
 *   with float atomics; run and mode 0 / 1 / 2 as in dvgo_vm_bwd (same defaults, same 64 KB table rule).  A sample whose
 *   grad_out[m] is exactly 0 (either sign) issues no atomic and does not end the run a lane is merging: it is passed over
 *   as if it were not there.  No gradient for xyz.
 * M == 0 or R == 0: no-op, no pointer is looked at.  DVGO_EINVAL: negative M, R or run, a plane axis or line length < 1,
 * a mode outside 0..2, null pointers, an explicit mode 2 whose table exceeds 64 KB.  DVGO_ERANGE: M * 3R >= 2^31 (the
 * lanes of the scatter at run 1; the forward, M lanes, is held to the same).  All of it is answered before any launch.
 * --------------------------------------------------------------------------------- */
int dvgo_vm_density_fwd(const float* xy, int H_xy, int W_xy, int64_t sC_xy, int64_t sH_xy, int64_t sW_xy,
                        const float* yz, int H_yz, int W_yz, int64_t sC_yz, int64_t sH_yz, int64_t sW_yz,
                        const float* zx, int H_zx, int W_zx, int64_t sC_zx, int64_t sH_zx, int64_t sW_zx,
                        const float* l_xy, int N_xy, int64_t lC_xy, int64_t lN_xy,
                        const float* l_yz, int N_yz, int64_t lC_yz, int64_t lN_yz,
                        const float* l_zx, int N_zx, int64_t lC_zx, int64_t lN_zx,
                        int R, const float* xyz, const float* xyz_min, const float* xyz_max, int64_t M, float* out,
                        void* stream);
int dvgo_vm_density_bwd(const float* grad_out,
                        const float* xy, int H_xy, int W_xy, int64_t sC_xy, int64_t sH_xy, int64_t sW_xy,
                        const float* yz, int H_yz, int W_yz, int64_t sC_yz, int64_t sH_yz, int64_t sW_yz,
                        const float* zx, int H_zx, int W_zx, int64_t sC_zx, int64_t sH_zx, int64_t sW_zx,
                        const float* l_xy, int N_xy, int64_t lC_xy, int64_t lN_xy,
                        const float* l_yz, int N_yz, int64_t lC_yz, int64_t lN_yz,
                        const float* l_zx, int N_zx, int64_t lC_zx, int64_t lN_zx,
                        float* g_xy, float* g_yz, float* g_zx, float* gl_xy, float* gl_yz, float* gl_zx,
                        int R, const float* xyz, const float* xyz_min, const float* xyz_max, int64_t M, int run, int mode,
                        void* stream);

/* ---------------------------------------------------------------------------------
 * Fused ray march over the VM decomposed density (csrc/march_vm.hip):
 * dvgo_march_density and dvgo_march_density_bwd with the dense grid replaced by the planes and lines of the block above.
 * Added without a bump of DVGO_ABI_VERSION, as that block was.
 * dvgo_march_vm_density: dvgo_march_density's contract -- one wavefront per ray, the same box test, occupancy lookup, alpha
 *   and weight filters, transmittance recurrence and stop, the same rec2 records, n2, n3 and alphainv_last, which
 *   dvgo_march_gather reads as they are -- with these differences:
 *     planes, lines, R in the argument order of dvgo_vm_density_fwd take the place of density, X, Y, Z;
 *     the ray setup always happens in this launch: rays_o, rays_d [N,3], near, far are inputs, rays_start, rays_dir [N,3] and
 *       n_steps [N] are OUTPUTS; records are at r * rec_stride only (rec_stride >= max n_steps; a ray whose step count
 *       exceeds it is marched up to rec_stride steps, never past its slice);
 *     stepdist must be > 0: NDC spacing is refused;
 *     no brick counters and no tail.
 *   xyz_min, xyz_max, xyz2ijk_scale, xyz2ijk_shift are HOST pointers, as in dvgo_march_density.  mask may be NULL.
 *   Per step s of ray r, all in float32, no contraction but where fmaf is written:
 *     p = fmaf(dir, stepdist * (float)s, start) per axis;  dropped when outside [xyz_min, xyz_max] or when its occupancy
 *       byte (index roundf(fmaf(p, scale, shift)) per axis, as dvgo_march_density) is 0;
 *     raw = dvgo_vm_density_fwd's chain at p: acc = 0; for s = xy, yz, zx: for r = 0 .. R - 1: acc = fmaf(p_{s,r}, l_{s,r},
 *       acc) -- the same bits as that entry gives for the same position, whatever the layout or alignment (16-byte loads
 *       under its rule, element loads otherwise);
 *     exp_d = expf(raw + act_shift), alpha = 1 - (1 + exp_d)^(-interval) (the power of dvgo_raw2alpha);
 *     T, the stop at T < 1e-3, the two filters and bit 31 of the record's step: as dvgo_march_density -- the occupancy
 *       index, the activation, the transmittance walk and the commit into the records are the functions that kernel calls
 *       (csrc/common.h: dvgo_mask_index; csrc/march_records.h), not copies of them.
 *   A chunk of 64 steps none of which passes box and mask reads no plane or line, and no chunk behind the ray's stop is
 *   visited.  Bitwise repeatable.
 * dvgo_march_vm_density_bwd: rec2, n2, n_steps, rec_stride, off3, rays_start, rays_dir, stepdist, alphainv_last, interval,
 *   grad_weights, grad_last as dvgo_march_density_bwd, from the same forward (n_steps is not read: the records are at
 *   r * rec_stride); off2 [N + 1] the exclusive scan of n2, M2 = off2[N].  The walk is dvgo_march_density_bwd's, the same
 *   function chunk by chunk (csrc/march_records.h owns it for every march): chunks of 64 records from the far end, rank of
 *   a flagged record from off3, the suffix sum of g_w * w over the lanes above by a shuffle tree, acc += the chunk's total,
 *   then
 *     g_alpha = (float)((double)(g_w * T) - (double)(acc + suffix) / ((double)(1 - alpha) + 1e-10))
 *     g_raw   = (float)(min((double)exp_d, 1e10) * (double)pow(1 + exp_d, -interval - 1) * interval * g_alpha)
 *   Record i of ray r writes g_raw[off2[r] + i] and its position xyz2[off2[r] + i] (the forward's expression: the same bits).
 *   Nothing is scattered: no atomics, no LDS, bitwise repeatable; every one of the M2 rows is written.  The gradients of
 *   planes and lines are dvgo_vm_density_bwd(g_raw, ..., xyz2, M2, ...), which passes over rows whose g_raw is exactly 0.
 * n_rays == 0: no-op.  DVGO_EINVAL: negative n_rays, R < 1, a plane axis or line length < 1, stepdist <= 0, rec_stride <= 0,
 * null pointers (grad_weights and grad_last may be NULL), a mask without its scale, shift or positive sizes.  DVGO_ERANGE:
 * n_rays * 64 or rec_stride >= 2^31.  All of it is answered before any launch.
 * --------------------------------------------------------------------------------- */
int dvgo_march_vm_density(float* rays_start, float* rays_dir, int64_t* n_steps, int64_t rec_stride, int64_t n_rays,
                          const float* xyz_min, const float* xyz_max, float stepdist,
                          const uint8_t* mask, int mX, int mY, int mZ,
                          const float* xyz2ijk_scale, const float* xyz2ijk_shift,
                          const float* xy, int H_xy, int W_xy, int64_t sC_xy, int64_t sH_xy, int64_t sW_xy,
                          const float* yz, int H_yz, int W_yz, int64_t sC_yz, int64_t sH_yz, int64_t sW_yz,
                          const float* zx, int H_zx, int W_zx, int64_t sC_zx, int64_t sH_zx, int64_t sW_zx,
                          const float* l_xy, int N_xy, int64_t lC_xy, int64_t lN_xy,
                          const float* l_yz, int N_yz, int64_t lC_yz, int64_t lN_yz,
                          const float* l_zx, int N_zx, int64_t lC_zx, int64_t lN_zx,
                          int R, float act_shift, float interval, float fast_color_thres,
                          dvgo_rec2_t* rec2, int32_t* n2, int32_t* n3, float* alphainv_last,
                          const float* rays_o, const float* rays_d, float near, float far, void* stream);
int dvgo_march_vm_density_bwd(const dvgo_rec2_t* rec2, const int32_t* n2, const int64_t* n_steps, int64_t rec_stride,
                              const int64_t* off3, const int64_t* off2, int64_t n_rays,
                              const float* rays_start, const float* rays_dir, float stepdist,
                              const float* alphainv_last, float interval,
                              const float* grad_weights /* [M3] */, const float* grad_last /* [N] or NULL */,
                              float* g_raw /* [M2] */, float* xyz2 /* [M2,3] */, void* stream);

/* dvgo_march_vm_ray_bwd: the gradient of dvgo_march_vm_density with respect to its RAYS (csrc/march_raygrad.hip;
 *   camera-pose refinement of TensoRFVoxGO on the fused march).  Added without a bump of
 *   DVGO_ABI_VERSION.  One wavefront per ray; records at r * rec_stride only, metric steps only, as that march.
 *   rec2, n2, rec_stride, off3, rays_start, rays_dir, stepdist, alphainv_last, interval, grad_weights, grad_last: as
 *   dvgo_march_vm_density_bwd, from the same forward; xyz_min, xyz_max HOST pointers; rays_o, rays_d, near, far: what the
 *   forward's ray setup read (t_min and |d| are recomputed by the same expressions); planes, lines, R in the argument order of
 *   dvgo_vm_density_fwd: they must hold what the forward read.  grad_pts [M3,3] in the M3 order of dvgo_march_gather: the
 *   gradient that arrived for the kept samples' positions, or NULL.
 *   The kernel does its own walk (dvgo_march_vm_density_bwd's, chunk by chunk the same function) and reads neither g_raw nor
 *   xyz2 of that entry: it runs when the model is frozen and that entry is never launched.  Per record, with g_raw as
 *   dvgo_march_vm_density_bwd would leave it and p = fmaf(rays_dir, dist, rays_start) (the forward's bits):
 *       (ox, oy, oz) = dvgo_vm_density_bwd_xyz's row at p for grad_out = g_raw: for s = xy, yz, zx: for r = 0 .. R - 1:
 *           t = g_raw * l, u = g_raw * p_;  Ah = fmaf(t, dh, Ah), Aw = fmaf(t, dw, Aw), An = fmaf(u, dn, An)
 *         with that entry's cell, weights, dropped corners and nodes (dh, dw the signed corner chains, dn = node1 - node0),
 *         then the plane's scale once -- Ah * ((float)(H - 1) / extent), likewise Aw, An -- added to the world axes the plane's
 *         rows, columns and line follow.  16-byte loads under dvgo_march_vm_density's rule, element loads otherwise: same bits.
 *       g_p = (ox, oy, oz);  for a kept record (index i in the M3 order), when grad_pts is given: g_p = g_p + grad_pts[3 i ..]
 *       lam = t_min + dist / |d|
 *   A record whose g_raw is exactly 0 and which has no pts term is passed over.  Per ray, dvgo_march_ray_bwd's sums in its
 *   order: grad_o[ray] = sum g_p, grad_d[ray] = sum (lam * g_p); plain stores by one lane, zeros for a ray without records;
 *   no atomics, no LDS, no workspace, bitwise repeatable.
 *   n_rays == 0: no-op, no pointer looked at.  DVGO_EINVAL: negative n_rays, R < 1, a plane axis or line length < 1,
 *   stepdist <= 0, rec_stride <= 0, then null pointers (grad_weights, grad_last and grad_pts may be NULL).  DVGO_ERANGE:
 *   n_rays * 64 or rec_stride >= 2^31. */
int dvgo_march_vm_ray_bwd(const dvgo_rec2_t* rec2, const int32_t* n2, int64_t rec_stride, const int64_t* off3,
                          int64_t n_rays, const float* rays_start, const float* rays_dir, float stepdist,
                          const float* xyz_min, const float* xyz_max, const float* alphainv_last, float interval,
                          const float* rays_o, const float* rays_d, float near, float far,
                          const float* xy, int H_xy, int W_xy, int64_t sC_xy, int64_t sH_xy, int64_t sW_xy,
                          const float* yz, int H_yz, int W_yz, int64_t sC_yz, int64_t sH_yz, int64_t sW_yz,
                          const float* zx, int H_zx, int W_zx, int64_t sC_zx, int64_t sH_zx, int64_t sW_zx,
                          const float* l_xy, int N_xy, int64_t lC_xy, int64_t lN_xy,
                          const float* l_yz, int N_yz, int64_t lC_yz, int64_t lN_yz,
                          const float* l_zx, int N_zx, int64_t lC_zx, int64_t lN_zx,
                          int R, const float* grad_weights /* [M3] */, const float* grad_last /* [N] or NULL */,
                          const float* grad_pts /* [M3,3] or NULL */, float* grad_o, float* grad_d, void* stream);

/* ---------------------------------------------------------------------------------
 * Fused ray march over the contracted space of unbounded scenes (csrc/march_contract.hip; INTEGRATION.md
 * section 5b): dvgo_contract_count / dvgo_contract_emit and dvgo_march_density in one launch.  Added without a bump of
 * DVGO_ABI_VERSION, as the block above was.
 * center, radius, xyz_min, xyz_max, xyz2ijk_scale, xyz2ijk_shift are HOST pointers (3 floats each), as in dvgo_march_density;
 * rays_o, rays_d [N,3], t_tab [n_max] and everything else are device pointers.  xyz_min / xyz_max are the CONTRACTED bounds
 * of the grids, -(1 + b) and 1 + b per axis for DirectContractedVoxGO.  mask may be NULL (all occupied).
 * dvgo_march_contract_density: one wavefront per ray, lanes = 64 consecutive steps k < n_max.  Per step, all in float32, no
 *   contraction but where fmaf is written, the sampler's expressions of the unbounded-scenes block operation for operation:
 *     o', d', p_k = o' + d' * t_tab[k], n_k, q_k = p_k if n_k <= 1 else (p_k / n_k) * ((1 + b) - b / n_k);
 *     k >= 1: acc = acc + sqrtf(ex ex + ey ey + ez ez), e = q_k - q_{k-1};  over_k = acc > thin_thres;  acc = 0 when over_k
 *       (acc = 0 before step 1; the adds happen in step order, across the 64 lanes of a chunk and from chunk to chunk: the
 *       kept set is dvgo_contract_emit's exactly);
 *     kept when (n_k <= 1 or over_k) and the occupancy byte at q_k (index roundf(fmaf(q, scale, shift)) per axis) is not 0;
 *     raw = the trilinear sample of density [X,Y,Z] (contiguous) at q_k over [xyz_min, xyz_max]: the bits dvgo_grid_sample_fwd
 *       gives at that position;  exp_d = expf(raw + act_shift), alpha = 1 - (1 + exp_d)^(-interval) (dvgo_raw2alpha's power,
 *       `interval` constant: stepsize * voxel_size_ratio);
 *     T, the stop at T < 1e-3, the two filters and bit 31 of the record's step (= k): as dvgo_march_density, through the
 *       same functions (csrc/march_records.h; the occupancy index: csrc/common.h, dvgo_mask_index).
 *   Records of ray r at rec2[r * rec_stride ...], rec_stride >= n_max.  n2, n3 [N] int32, alphainv_last [N].
 *   A chunk in which no step is kept reads no density, and no chunk behind the ray's stop is visited (the thinning walk runs
 *   in every chunk that is visited).  Bitwise repeatable.
 * dvgo_march_contract_density_bwd: the walk of dvgo_march_vm_density_bwd over the same records, the same g_alpha and g_raw
 *   expressions (csrc/march_records.h is their one copy, dvgo_march_density_bwd's too).  Record i of ray r writes
 *   g_raw[off2[r] + i] and its contracted position q2[off2[r] + i] = q_k of its step, the forward's bits.  off3 / off2
 *   [N + 1]: exclusive scans of n3 / n2.  Nothing is scattered: no atomics, no LDS, bitwise repeatable, every one of the M2
 *   rows written.  The gradient of the grid is dvgo_grid_sample_bwd(g_raw, C = 1, ..., q2, xyz_min, xyz_max, M2, ...).
 * dvgo_contract_positions: elementwise over M pairs (ray_id, step_id): q [M,3] = q_k and t [M] = t_tab[k], the bits
 *   dvgo_contract_emit writes for that ray and step.  A pair outside [0, n_rays) x [0, n_max) reads nothing and gets NaN.
 * n_rays == 0 (M == 0): no-op.  DVGO_EINVAL: negative n_rays or M, n_max <= 0, rec_stride < n_max, X, Y or Z <= 0, null
 * pointers (grad_weights and grad_last may be NULL), a mask without its scale, shift or positive sizes.  DVGO_ERANGE:
 * n_rays * 64, rec_stride, X * Y * Z or M >= 2^31.  All of it is answered before any launch.
 * --------------------------------------------------------------------------------- */
int dvgo_march_contract_density(const float* rays_o, const float* rays_d, int64_t n_rays, const float* center,
                                const float* radius, const float* t_tab, int n_max, float bg_len, int l2, float thin_thres,
                                const uint8_t* mask, int mX, int mY, int mZ, const float* xyz2ijk_scale,
                                const float* xyz2ijk_shift, const float* density, int X, int Y, int Z, const float* xyz_min,
                                const float* xyz_max, float act_shift, float interval, float fast_color_thres,
                                int64_t rec_stride, dvgo_rec2_t* rec2, int32_t* n2, int32_t* n3, float* alphainv_last,
                                void* stream);
int dvgo_march_contract_density_bwd(const dvgo_rec2_t* rec2, const int32_t* n2, int64_t rec_stride, const int64_t* off3,
                                    const int64_t* off2, int64_t n_rays, const float* rays_o, const float* rays_d,
                                    const float* center, const float* radius, const float* t_tab, int n_max, float bg_len,
                                    int l2, const float* alphainv_last, float interval, const float* grad_weights,
                                    const float* grad_last, float* g_raw, float* q2, void* stream);
int dvgo_contract_positions(const float* rays_o, const float* rays_d, int64_t n_rays, const float* center,
                            const float* radius, const float* t_tab, int n_max, float bg_len, int l2,
                            const int64_t* ray_id, const int64_t* step_id, int64_t M, float* q, float* t, void* stream);

/* ---------------------------------------------------------------------------------
 * The contraction's ray gradient (csrc/contract_raygrad.hip): from dL/dq of
 * the kept samples of the contracted space to dL/d rays_o and dL/d rays_d, summed per ray.  Camera-pose refinement of
 * unbounded scenes.  Added without a bump of DVGO_ABI_VERSION, as the blocks above were.
 * center, radius: HOST pointers (3 floats each); everything else is a device pointer.  rays_o, rays_d [N,3], t_tab [n_max],
 * bg_len (b), l2: what the forward (dvgo_contract_emit, dvgo_march_contract_density) was given.
 * The samples of ray r, in two forms that share one device body:
 *   dvgo_contract_ray_bwd      rows off[r] .. off[r + 1] - 1 of grad_q [M,3] and step_id [M] (a ray-major list; off [N + 1]
 *                              ascending).  off is clamped to [0, M]: no row outside grad_q is read.
 *   dvgo_contract_ray_bwd_rec  the records of the fused march: record i < n2[r] of ray r is rec2[r * rec_stride + i], its step
 *                              rec.step & 0x7fffffff, its row of grad_q2 [M2,3] is off2[r] + i (the rows
 *                              dvgo_march_contract_density_bwd writes).  A ray whose rows would leave [0, M2) reads none of
 *                              them and gets NaN.
 * One wavefront per ray; lanes take 64 consecutive samples per chunk, chunks ascending.  Per sample with step k and row g,
 * all in float32, no contraction, division and square root correctly rounded:
 *     o', d', ||u||, p = o' + d' * t_tab[k], n: the forward's expressions and bits (csrc/contract_common.h), so `n <= 1` and
 *       the arg-max axis are the forward's own choices
 *     n <= 1 (n == 1 included):  h = g
 *     n  > 1:  f  = ((1 + b) - b / n) / n;   f' = ((2 * b) / n - (1 + b)) / (n * n);   c = f' * ((px * gx + py * gy) + pz * gz)
 *              l2 != 0:  h_a = f * g_a + (p_a / n) * c          for every axis a
 *              l2 == 0:  h_a = f * g_a + (p_a < 0 ? -c : c)     for a = the LOWEST axis index with |p_a| == max|p|
 *                        h_a = f * g_a                          for the other two
 *     A = A + h;   B = B + t_tab[k] * h        (six accumulators per lane, carried across the chunks)
 *   g == 0 contributes exact zeros.  After the last chunk one butterfly over the 64 lanes (v += shfl_xor(v, d), d = 32, 16,
 *   .. 1) sums each accumulator, and one lane writes, with plain stores,
 *     grad_o[r] = A / radius
 *     grad_d[r] = ((B - d' * ((d'x * Bx + d'y * By) + d'z * Bz)) / ||u||) / radius      (the normalisation of d is differentiated:
 *                                                                                        t_tab is a true constant)
 *   A ray without samples gets exact zeros.  A step outside [0, n_max) reads nothing and makes both outputs of its ray NaN.
 *   No atomics, no LDS, no workspace, nothing to zero beforehand: bitwise repeatable.
 * n_rays == 0: no-op.  DVGO_EINVAL: negative n_rays, M, M2 or rec_stride, n_max <= 0, null pointers (grad_q / step_id, grad_q2 /
 * rec2 may be NULL when M, M2 == 0).  DVGO_ERANGE: n_rays * 64 or rec_stride >= 2^31.  All of it is answered before any launch.
 * --------------------------------------------------------------------------------- */
int dvgo_contract_ray_bwd(const float* rays_o, const float* rays_d, int64_t n_rays, const float* center,
                          const float* radius, const float* t_tab, int n_max, float bg_len, int l2, const float* grad_q,
                          const int64_t* step_id, int64_t M, const int64_t* off, float* grad_o, float* grad_d,
                          void* stream);
int dvgo_contract_ray_bwd_rec(const float* rays_o, const float* rays_d, int64_t n_rays, const float* center,
                              const float* radius, const float* t_tab, int n_max, float bg_len, int l2,
                              const dvgo_rec2_t* rec2, const int32_t* n2, int64_t rec_stride, const int64_t* off2,
                              const float* grad_q2, int64_t M2, float* grad_o, float* grad_d, void* stream);

/* ---------------------------------------------------------------------------------
 * Total-variation and L1 regularisers of plane-shaped parameters, added to their gradients (csrc/plane_tv.hip; DESIGN.md
 * section 6k).  The 2-D counterpart of dvgo_total_variation_add_grad for the feature planes
 * [1,C,H,W] and lines [1,R,N,1] of the tri-plane models: up to 8 tensors in ONE launch.
 * HOST tables, one entry per tensor t < n_tensors (as dvgo_copy_multi / dvgo_adam_upd_multi):
 *   params[t], grads[t]   device pointers of a parameter and of its gradient, which share the strides below
 *   sizes[3t .. 3t+2]     C, H, W, each at least 1
 *   strides[3t .. 3t+2]   sC, sH, sW in ELEMENTS: any dense layout (the models store channels-last: sC = 1, sW = C, sH = W C)
 *   weights[3t .. 3t+2]   wh, ww, wl1, already normalised by the caller: the kernel divides nothing
 * A line [1,R,N,1] is a tensor with W == 1: its column terms vanish by themselves.
 * Per element o = c sC + h sH + w sW, all in float32, no contraction, in exactly this order (the 3-D kernel's: innermost
 * axis first), clamp1(v) = fminf(fmaxf(v, -1), 1):
 *   if (!dense_mode && grad[o] == 0.0f)  grad[o] stays untouched (a -0.0 stays -0.0)
 *   p = param[o];  g = 0
 *   if (w > 0)      g = g + ww * clamp1(p - param[o - sW])
 *   if (w < W - 1)  g = g + ww * clamp1(p - param[o + sW])
 *   if (h > 0)      g = g + wh * clamp1(p - param[o - sH])
 *   if (h < H - 1)  g = g + wh * clamp1(p - param[o + sH])
 *   if (wl1 != 0)   g = g + wl1 * sgn(p)                        sgn(+-0) = 0
 *   grad[o] = grad[o] + g
 * (a boundary term may instead be multiplied by a zero weight on a clamped in-bounds load: bit-equal for finite
 * parameters; non-finite parameters are outside the contract).  No atomics: bitwise repeatable.  With wl1 = 0 and
 * wh = ww = w / 6 this is dvgo_total_variation_add_grad(wy = wz = w) on the same memory viewed as [1,C,1,H,W], bit for bit.
 * A workgroup owns one contiguous row of one tensor (channels-last: the W C floats of one h; channel-first: the W floats of
 * one (c, h); any other layout goes through the strides), found through a prefix table that travels with the launch.
 * n_tensors == 0: no-op, no table is looked at.  DVGO_EINVAL: n_tensors < 0 or > 8, a null table, a size below 1, a null
 * params[t] or grads[t].  DVGO_ERANGE: a tensor of 2^31 elements or more, or 2^31 rows or more in all.  All of it is
 * answered before any launch.
 * --------------------------------------------------------------------------------- */
int dvgo_plane_reg_add_grad(const float* const* params, float* const* grads, const int64_t* sizes,
                            const int64_t* strides, const float* weights, int n_tensors, int dense_mode, void* stream);

/* ---------------------------------------------------------------------------------
 * Multiresolution hash-grid features (csrc/hashgrid.hip).  The encoding
 * of Instant-NGP (Mueller et al., SIGGRAPH 2022): L trilinear lattices of growing resolution whose nodes are rows of ONE
 * table.  No counterpart in the reference; the contract is this text.
 *   table    fp32 [T_total, F], contiguous, F in {1, 2, 4, 8}, aligned to min(4 F, 16) bytes (as are out, grad_out, grad_table)
 *   res      HOST int32 [L, 3]: the node counts (Rx, Ry, Rz) of level l along the world axes, each at least 2
 *   offsets  HOST int64 [L + 1], offsets[0] >= 0: the first row of every level; size_l = offsets[l + 1] - offsets[l]
 *            size_l == Rx Ry Rz: level l is DENSE.  Otherwise it is HASHED and size_l must be a power of two below Rx Ry Rz.
 *   1 <= L <= DVGO_HASH_MAX_LEVELS.
 * Per sample m, level l and axis a, all in float32, no contraction:
 *   g = ((((p_a - min_a) / (max_a - min_a)) * 2 - 1) + 1) / 2 * (R_a - 1)          (the library's align_corners=True coordinate)
 *   g = fminf(fmaxf(g, 0), R_a - 1);   f = min((int)floorf(g), R_a - 2);   w0 = (f + 1) - g;   w1 = g - f
 * so a position outside the box reads the box's face (no zero padding) and all eight corners exist.  Corner n = 0..7 is
 * (fx + (n >> 2 & 1), fy + (n >> 1 & 1), fz + (n & 1)): x slowest, z fastest; its weight is (wx * wy) * wz.  Its row:
 *   dense    (ix Ry + iy) Rz + iz
 *   hashed   ((uint32)ix * 1u ^ (uint32)iy * 2654435761u ^ (uint32)iz * 805459861u) & (size_l - 1), wrapping 32-bit products
 * dvgo_hash_fwd: xyz [M,3] world coordinates, xyz_min / xyz_max device float[3] -> out [M, L F]:
 *   out[m, l F + c] = acc after acc = 0; acc = fmaf(table[offsets[l] + row_n, c], w_n, acc) for n = 0..7.  Bitwise repeatable.
 * dvgo_hash_bwd: grad_out [M, L F] and a buffer grad_table [T_total, F] (zero-filled or holding a partial sum):
 *   grad_table[offsets[l] + row_n, c] += w_n * grad_out[m, l F + c]
 *   with float atomics: the summation order is not reproducible.  Two corners of one cell that share a row both add.  The
 *   table's values are not read.  No gradient for xyz.
 *   mode 1: a lane owns `run` consecutive samples of one level and sums the 8 F corner terms in registers while the samples
 *     stay in one cell, before its atomics (run 1: nothing merged; 0: the library's default).  mode 2: one lane per (sample,
 *     level, corner), nothing merged, run ignored.  mode 3: mode 1 with the F channels of a row on F neighbouring lanes (a lane
 *     owns run, level and channel): one atomic instruction adds whole rows.  mode 0: the library's choice
 *     (profiles/hash/README.md).
 * M == 0: no-op, no device pointer is looked at (the level table is still checked).  DVGO_EINVAL: F outside {1,2,4,8}, L outside
 * 1..DVGO_HASH_MAX_LEVELS, a node count below 2, offsets[0] < 0, a size_l that is neither the node count nor a power of two
 * below it, negative M or run, a mode outside 0..3, null or misaligned pointers.  DVGO_ERANGE: M L F >= 2^31 (mode 2:
 * 8 M L >= 2^31), Rx Ry >= 2^31, a hashed level of more than 2^31 rows.  All of it is answered before any launch.
 *
 * dvgo_hash_bwd_xyz (csrc/hash_xyz.hip): the gradient of the features with respect to the sample POSITION, which
 * dvgo_hash_bwd does not give.  table [T_total, F] (its values are read), grad_out [M, L F], xyz [M,3] -> grad_xyz [M,3].
 * Every row of grad_xyz is written with plain stores: no atomics, no workspace, nothing to zero beforehand.  F, L, res,
 * offsets and the alignment of table and grad_out are dvgo_hash_fwd's (grad_xyz: a float's).  Added without a bump of
 * DVGO_ABI_VERSION, as the two entries above were.
 * The cell (fx, fy, fz) and the weights w0, w1 of every axis are the forward's own, bit for bit, so the derivative is that of
 * the cell the forward chose: floorf picks the upper cell on an interior lattice plane, f = min(floor, R - 2) the last cell
 * at g == R - 1.  The forward clamps the coordinate, so outside the box the features are constant along the clamped axis:
 * with inside_a = (g_a >= 0) & (g_a <= R_a - 1) on the UNCLAMPED float32 g_a (a NaN is not inside), level l contributes
 * exactly 0.0f along axis a when !inside_a; the other axes keep theirs.
 * Per sample m, in float32, one lane, everything in this order whatever the launch shape (bitwise repeatable):
 *   ox = oy = oz = 0.0f
 *   for l = 0 .. L - 1 ascending:
 *     the two-weight product of corner n = 0..7 (bx = n >> 2 & 1, by = n >> 1 & 1, bz = n & 1), first factor * second:
 *       for d/dx  wy[by] * wz[bz]      for d/dy  wx[bx] * wz[bz]      for d/dz  wx[bx] * wy[by]
 *     negated on the lower corner of the derivative's axis (b = 0) and as it is on the upper (b = 1): sx_n, sy_n, sz_n (exact)
 *     ax = ay = az = 0.0f
 *     for c = 0 .. F - 1 ascending:
 *       dx = dy = dz = 0.0f;  for n = 0 .. 7 ascending, v = table[offsets[l] + row_n, c]:
 *         dx = fmaf(v, sx_n, dx);  dy = fmaf(v, sy_n, dy);  dz = fmaf(v, sz_n, dz)
 *       ax = fmaf(grad_out[m, l F + c], dx, ax);  ay, az likewise
 *     the level's scale is applied once, after the last channel:  tx = ax * ((float)(Rx_l - 1) / (max_x - min_x)), ty, tz likewise
 *     ox = ox + (inside_x ? tx : 0.0f);  oy, oz likewise
 *   grad_xyz[m] = (ox, oy, oz)
 * Two corners of one cell that share a row of a hashed level are two terms, as in the forward.
 * M == 0: no-op, no device pointer is looked at (the level table is still checked).  DVGO_EINVAL and DVGO_ERANGE as for
 * dvgo_hash_fwd, for the same conditions in the same order; all of it is answered before any launch.
 * --------------------------------------------------------------------------------- */
#define DVGO_HASH_MAX_LEVELS 32
int dvgo_hash_fwd(const float* table, int F, int L, const int32_t* res, const int64_t* offsets, const float* xyz,
                  const float* xyz_min, const float* xyz_max, int64_t M, float* out, void* stream);
int dvgo_hash_bwd(const float* grad_out, float* grad_table, int F, int L, const int32_t* res, const int64_t* offsets,
                  const float* xyz, const float* xyz_min, const float* xyz_max, int64_t M, int run, int mode, void* stream);
int dvgo_hash_bwd_xyz(const float* table, int F, int L, const int32_t* res, const int64_t* offsets,
                      const float* grad_out, const float* xyz, const float* xyz_min, const float* xyz_max,
                      int64_t M, float* grad_xyz, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DVGO_HIP_H */
