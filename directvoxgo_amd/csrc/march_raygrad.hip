// The derivative of the fused marches with respect to their RAYS (camera-pose refinement on the fused path: pose.py,
// INTEGRATION.md section 7, DESIGN.md sections 6h and 6p).  Three kernels, one walk:
//
//   march_ray_bwd         the dense density grid and a k0 colour grid (fused_march: DirectVoxGO).  Per record
//                             g_p = scale * (g_d * d density / d g  +  [kept] sum_c grad_feat[off3[ray] + rank, c] * d k0_c / d g)
//                         (the corner chains of dvgo_grid_sample_bwd_xyz, xyz_corners.h: the density grid as the first
//                         channel, then, for a record that survived into the M3 arrays, the feature channels ascending).
//   march_pts_ray_bwd     the dense density grid, positions handed to the caller (fused_march(positions=True): HashVoxGO,
//                         VMTriPlaneVoxGO): the k0 term replaced by the gradient that arrived for the kept samples' positions,
//                             g_p = scale * (g_d * d density / d g)  +  [kept] grad_pts[off3[ray] + rank]
//   march_vm_ray_bwd      the decomposed density (fused_march_vm: TensoRFVoxGO), over the records of march_vm_density,
//                             g_p = g_raw * d(sum_{s,r} plane_{s,r} * line_{s,r}) / d xyz  +  [kept] grad_pts[off3[ray] + rank]
//                         with the position derivative of vm_xyz.hip's density entry (vm_common.h: vm_xyz): its cell, weights,
//                         dropped corners and nodes, component order and per-plane scale.
//
// march_ray_bwd_walk is all three: one wavefront per ray; the ray's rec2 records from the far end in chunks of 64 through
// march_bwd_chunk (march_records.h: the walk of every march backward); the record's position from the forward's expression
// fmaf(dir, march_dist(stepdist, step), start), hence its bits; lam = t_min + dist / |d| a constant of the derivative;
//     grad_o[ray] = sum g_p        grad_d[ray] = sum lam * g_p
// in float32, a butterfly over the 64 lanes per chunk (lanes without a record add 0), chunks far to near into one
// accumulator per component: a fixed order, so the result is bitwise repeatable.  Lane 0 writes both rows with plain stores,
// zeros for a ray without records: no atomics, no LDS, no workspace, nothing to zero beforehand.  No kernel reads what the
// density backward of its march leaves behind (g_raw, xyz2): each does its own walk, so a frozen model, whose density
// backward never runs, still moves its cameras.  include/dvgo_hip.h states the arithmetic.
#include "march_records.h"
#include "vm_common.h"
#include "xyz_corners.h"

struct RayGradParams {
  float mnx, mny, mnz, mxx, mxy, mxz;
  float stepdist;          // > 0
  int X, Y, Z;             // the density lattice (the dense kernels only)
  float interval;
};

// The walk.  What a kernel adds per record is its `term`:
//   term.begin(o3)                                       once, by a ray that has records: o3 = off3[ray], the ray's first row
//                                                        of the M3 arrays
//   term(px, py, pz, g_d, flag, rank, gx, gy, gz)        the record at (px, py, pz) with the raw-density gradient g_d, kept
//                                                        (`flag`) as number `rank` of the ray's kept samples: false when the
//                                                        record contributes nothing, else g_p in (gx, gy, gz)
// lam is formed only for a record that contributes: a skipped one keeps adding exact zeros, where 0 * lam would be NaN for a
// ray with |d| = 0.  n_steps / cum may be NULL: the records are then at ray * rec_stride (rec_base).
// LANE_ROWS: the ray's own rows (records, weight gradients, outputs) as per-lane addresses in vector registers, for a
// kernel whose arguments leave few scalar ones (the VM kernel: three planes and three lines by value; held in scalar
// registers across the walk these pointers were spilled: profiles/march_pts_raygrad/README.md).
template <bool LANE_ROWS, class Term>
__device__ __forceinline__ void march_ray_bwd_walk(const dvgo_rec2_t* __restrict__ rec2, const int32_t* __restrict__ n2,
                                                   const int64_t* __restrict__ n_steps, const int64_t* __restrict__ cum,
                                                   int64_t rec_stride, const int64_t* __restrict__ off3, int64_t n_rays,
                                                   const float* __restrict__ rays_start, const float* __restrict__ rays_dir,
                                                   const RayGradParams& P, const float* __restrict__ alphainv_last,
                                                   const float* __restrict__ rays_o, const float* __restrict__ rays_d, float near,
                                                   float far, const float* __restrict__ grad_weights,
                                                   const float* __restrict__ grad_last, float* __restrict__ grad_o,
                                                   float* __restrict__ grad_d, Term term) {
  const int64_t ray = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (ray >= n_rays) return;
  const int c2 = __builtin_amdgcn_readfirstlane(n2[ray]);
  float* __restrict__ out_o = grad_o + 3 * ray;
  float* __restrict__ out_d = grad_d + 3 * ray;
  if constexpr (LANE_ROWS) asm volatile("" : "+v"(out_o), "+v"(out_d));
  float Ax = 0.f, Ay = 0.f, Az = 0.f, Bx = 0.f, By = 0.f, Bz = 0.f;
  if (c2 > 0) {
    const int64_t o3 = off3[ray];
    int c3_rem = (int)(off3[ray + 1] - o3);
    // (march_bwd_chunk gets the ray's first record and first weight gradient, and 0 offsets)
    const dvgo_rec2_t* __restrict__ recs = rec2 + rec_base(cum, n_steps, rec_stride, ray);
    const float* __restrict__ gws = grad_weights + o3;
    if constexpr (LANE_ROWS) asm volatile("" : "+v"(recs), "+v"(gws));
    term.begin(o3);
    const float sx = rays_start[3 * ray], sy = rays_start[3 * ray + 1], sz = rays_start[3 * ray + 2];
    const float dx = rays_dir[3 * ray], dy = rays_dir[3 * ray + 1], dz = rays_dir[3 * ray + 2];
    const RaySetup S = dvgo_ray_setup(rays_o[3 * ray], rays_o[3 * ray + 1], rays_o[3 * ray + 2], rays_d[3 * ray], rays_d[3 * ray + 1],
                                      rays_d[3 * ray + 2], P.mnx, P.mny, P.mnz, P.mxx, P.mxy, P.mxz, near, far, P.stepdist);
    const unsigned long long lt = lanemask_lt(lane);
    float acc = (grad_last ? grad_last[ray] : 0.0f) * alphainv_last[ray];
    for (int hi = c2; hi > 0; hi -= 64) {
      const int lo = max(0, hi - 64);
      const MarchBwdChunk ck = march_bwd_chunk(recs, 0, lo, hi - lo, lane, lt, 0, c3_rem, acc, gws);
      const bool act = ck.act, flag = ck.flag;
      const int step = ck.step, rank = ck.rank;
      float gx = 0.f, gy = 0.f, gz = 0.f, lam = 0.f;
      if (act) {
        const float g_d = ck.g_d(P.interval);
        const float dist = march_dist(P.stepdist, step);
        const float px = fmaf(dx, dist, sx), py = fmaf(dy, dist, sy), pz = fmaf(dz, dist, sz);
        if (term(px, py, pz, g_d, flag, rank, gx, gy, gz)) lam = S.tmin + dist / S.rnorm;
      }
      Ax += wave_sum(gx); Ay += wave_sum(gy); Az += wave_sum(gz);
      Bx += wave_sum(lam * gx); By += wave_sum(lam * gy); Bz += wave_sum(lam * gz);
    }
  }
  if (lane == 0) {
    out_o[0] = Ax; out_o[1] = Ay; out_o[2] = Az;
    out_d[0] = Bx; out_d[1] = By; out_d[2] = Bz;
  }
}

// the gradient that arrived for a kept record's position: row `rank` of the ray's rows of grad_pts
struct PtsRow {
  float x = 0.f, y = 0.f, z = 0.f;
  __device__ __forceinline__ void load(const float* __restrict__ rows, int rank) {
    const float* __restrict__ g = rows + rank * 3;
    x = g[0]; y = g[1]; z = g[2];
  }
  __device__ __forceinline__ void add(float& gx, float& gy, float& gz) const { gx = gx + x; gy = gy + y; gz = gz + z; }
};

// The dense density grid's term.  KVEC = 4 / 1: with the k0 grid's channels, `rows` = grad_feat [M3, C] (4: k0
// channels-last with C % 4 == 0 and 16-byte aligned k0 / grad_feat: the eight corner rows of a channel group travel as
// float4s in flight together; 1: element strides, one channel at a time).  KVEC = 0: no colour grid, `rows` = grad_pts
// [M3, 3].  `rows` NULL: the density alone.
template <int KVEC>
struct DenseTerm {
  RayGradParams P;
  const float* __restrict__ density;
  const float* __restrict__ rows;
  const float* __restrict__ k0;
  int C;
  int64_t sC, sX, sY, sZ;
  bool has;
  float scale_x, scale_y, scale_z;

  __device__ __forceinline__ void begin(int64_t o3) {
    has = rows != nullptr && (KVEC == 0 || C > 0);
    rows += o3 * (KVEC == 0 ? 3 : C);
    scale_x = (float)(P.X - 1) / (P.mxx - P.mnx);
    scale_y = (float)(P.Y - 1) / (P.mxy - P.mny);
    scale_z = (float)(P.Z - 1) / (P.mxz - P.mnz);
  }

  __device__ __forceinline__ bool operator()(float px, float py, float pz, float g_d, bool flag, int rank, float& gx, float& gy,
                                             float& gz) const {
    const TriSetup t = dvgo_tri_setup(px, py, pz, P.mnx, P.mny, P.mnz, P.mxx, P.mxy, P.mxz, P.X, P.Y, P.Z);
    const bool extra = flag && has;
    if (!(g_d != 0.0f || extra)) return false;          // exact zeros, no loads
    const XyzCorners k = dvgo_xyz_corners(t, P.X, P.Y, P.Z, (int64_t)P.Y * P.Z, (int64_t)P.Z, 1);     // offsets: the density grid's
    float ax = 0.f, ay = 0.f, az = 0.f;
    PtsRow q;
    {
      float dv[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) dv[c] = density[k.off[c]];
      if constexpr (KVEC == 0)
        if (extra) q.load(rows, rank);                  // in flight with the corners
      // (keeps hipcc from sinking each load to its corner's fmaf: profiles/raygrad/README.md)
      __builtin_amdgcn_sched_barrier(0);
      DVGO_XYZ_CHANNEL(dv[n], g_d);
    }
    if constexpr (KVEC != 0) {
      if (extra) {
        int64_t koff[8];                                // the same clamped corners in k0's strides
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const int i = min(max(t.i0 + ((c >> 2) & 1), 0), P.X - 1);
          const int j = min(max(t.j0 + ((c >> 1) & 1), 0), P.Y - 1);
          const int kk = min(max(t.k0 + (c & 1), 0), P.Z - 1);
          koff[c] = (int64_t)i * sX + (int64_t)j * sY + (int64_t)kk * sZ;
        }
        const float* __restrict__ grow = rows + rank * (int64_t)C;
        if constexpr (KVEC == 4) {
          for (int c = 0; c < C; c += 4) {
            float4 fv[8];
#pragma unroll
            for (int n = 0; n < 8; ++n) fv[n] = *reinterpret_cast<const float4*>(k0 + koff[n] + c);
            const float4 g = *reinterpret_cast<const float4*>(grow + c);
            __builtin_amdgcn_sched_barrier(0);
            DVGO_XYZ_CHANNEL(fv[n].x, g.x);
            DVGO_XYZ_CHANNEL(fv[n].y, g.y);
            DVGO_XYZ_CHANNEL(fv[n].z, g.z);
            DVGO_XYZ_CHANNEL(fv[n].w, g.w);
          }
        } else {
          for (int c = 0; c < C; ++c) {
            float fv[8];
#pragma unroll
            for (int n = 0; n < 8; ++n) fv[n] = k0[c * sC + koff[n]];
            const float g = grow[c];
            DVGO_XYZ_CHANNEL(fv[n], g);
          }
        }
      }
    }
    gx = ax * scale_x; gy = ay * scale_y; gz = az * scale_z;
    if constexpr (KVEC == 0)
      if (extra) q.add(gx, gy, gz);
    return true;
  }
};

// The decomposed density's term: vm_xyz with the raw-density gradient for all 3R products, then the kept record's row of
// grad_pts.  VEC = 4: R % 4 == 0, channels-last, 16-byte aligned planes and lines (march_vm_density's rule); VEC = 1:
// everything else.  Same chains, same bits.
template <int VEC>
struct VmTerm {
  RayGradParams P;
  TpPlane QA, QB, QC;
  VmLine MA, MB, MC;
  int R;
  const float* __restrict__ rows;      // grad_pts [M3, 3] or NULL
  bool has;

  __device__ __forceinline__ void begin(int64_t o3) {
    has = rows != nullptr;
    rows += 3 * o3;
    asm volatile("" : "+v"(rows));     // (the walk's LANE_ROWS)
    // Likewise the 15 strides of planes and lines (30 scalar registers): they only ever multiply a lane's own corner or
    // node index, so they live in vector registers from here on.  Same values, same selects (tp_pick, vm_pick).
    asm volatile("" : "+v"(QA.sC), "+v"(QA.sH), "+v"(QA.sW), "+v"(QB.sC), "+v"(QB.sH), "+v"(QB.sW), "+v"(QC.sC), "+v"(QC.sH),
                 "+v"(QC.sW));
    asm volatile("" : "+v"(MA.sC), "+v"(MA.sN), "+v"(MB.sC), "+v"(MB.sN), "+v"(MC.sC), "+v"(MC.sN));
  }

  __device__ __forceinline__ bool operator()(float px, float py, float pz, float g_raw, bool flag, int rank, float& gx, float& gy,
                                             float& gz) const {
    const bool pts = flag && has;
    if (!(g_raw != 0.0f || pts)) return false;          // the record is passed over
    PtsRow q;
    if (pts) q.load(rows, rank);
    if (g_raw != 0.0f) {
      const float p[3] = {px, py, pz};
      const float mn[3] = {P.mnx, P.mny, P.mnz}, mx[3] = {P.mxx, P.mxy, P.mxz};
      vm_xyz<VEC>(QA, QB, QC, MA, MB, MC, R, p, mn, mx, VmGradScalar{g_raw}, gx, gy, gz);
    }
    if (pts) q.add(gx, gy, gz);
    return true;
  }
};

template <int VEC>
__global__ void __launch_bounds__(DVGO_BLOCK)
march_ray_bwd_kernel(const dvgo_rec2_t* __restrict__ rec2, const int32_t* __restrict__ n2,
                     const int64_t* __restrict__ n_steps, const int64_t* __restrict__ cum,
                     int64_t rec_stride, const int64_t* __restrict__ off3, int64_t n_rays,
                     const float* __restrict__ rays_start, const float* __restrict__ rays_dir,
                     RayGradParams P, const float* __restrict__ alphainv_last,
                     const float* __restrict__ rays_o, const float* __restrict__ rays_d, float near, float far,
                     const float* __restrict__ density, const float* __restrict__ k0, int C, int64_t sC, int64_t sX,
                     int64_t sY, int64_t sZ, const float* __restrict__ grad_weights,
                     const float* __restrict__ grad_last, const float* __restrict__ grad_feat,
                     float* __restrict__ grad_o, float* __restrict__ grad_d) {
  march_ray_bwd_walk<false>(rec2, n2, n_steps, cum, rec_stride, off3, n_rays, rays_start, rays_dir, P, alphainv_last, rays_o, rays_d,
                            near, far, grad_weights, grad_last, grad_o, grad_d,
                            DenseTerm<VEC>{P, density, grad_feat, k0, C, sC, sX, sY, sZ});
}

__global__ void __launch_bounds__(DVGO_BLOCK)
march_pts_ray_bwd_kernel(const dvgo_rec2_t* __restrict__ rec2, const int32_t* __restrict__ n2,
                         const int64_t* __restrict__ n_steps, const int64_t* __restrict__ cum, int64_t rec_stride,
                         const int64_t* __restrict__ off3, int64_t n_rays, const float* __restrict__ rays_start,
                         const float* __restrict__ rays_dir, RayGradParams P, const float* __restrict__ alphainv_last,
                         const float* __restrict__ rays_o, const float* __restrict__ rays_d, float near, float far,
                         const float* __restrict__ density, const float* __restrict__ grad_weights,
                         const float* __restrict__ grad_last, const float* __restrict__ grad_pts,
                         float* __restrict__ grad_o, float* __restrict__ grad_d) {
  march_ray_bwd_walk<false>(rec2, n2, n_steps, cum, rec_stride, off3, n_rays, rays_start, rays_dir, P, alphainv_last, rays_o, rays_d,
                            near, far, grad_weights, grad_last, grad_o, grad_d, DenseTerm<0>{P, density, grad_pts});
}

template <int VEC>
__global__ void __launch_bounds__(DVGO_BLOCK)
march_vm_ray_bwd_kernel(TpPlane PA, TpPlane PB, TpPlane PC, VmLine LA, VmLine LB, VmLine LC, int R,
                        const dvgo_rec2_t* __restrict__ rec2, const int32_t* __restrict__ n2, int64_t rec_stride,
                        const int64_t* __restrict__ off3, int64_t n_rays, const float* __restrict__ rays_start,
                        const float* __restrict__ rays_dir, RayGradParams P, const float* __restrict__ alphainv_last,
                        const float* __restrict__ rays_o, const float* __restrict__ rays_d, float near, float far,
                        const float* __restrict__ grad_weights, const float* __restrict__ grad_last,
                        const float* __restrict__ grad_pts, float* __restrict__ grad_o, float* __restrict__ grad_d) {
  march_ray_bwd_walk<true>(rec2, n2, nullptr, nullptr, rec_stride, off3, n_rays, rays_start, rays_dir, P, alphainv_last, rays_o,
                           rays_d, near, far, grad_weights, grad_last, grad_o, grad_d,
                           VmTerm<VEC>{P, PA, PB, PC, LA, LB, LC, R, grad_pts});
}

static RayGradParams ray_grad_params(const float* mn, const float* mx, float stepdist, int X, int Y, int Z, float interval) {
  RayGradParams P;
  P.mnx = mn[0]; P.mny = mn[1]; P.mnz = mn[2];
  P.mxx = mx[0]; P.mxy = mx[1]; P.mxz = mx[2];
  P.stepdist = stepdist;
  P.X = X; P.Y = Y; P.Z = Z;
  P.interval = interval;
  return P;
}

extern "C" {

// NOTE: xyz_min / xyz_max are HOST pointers (3 floats each), as in march.hip's and march_vm.hip's entries.

int dvgo_march_ray_bwd(const dvgo_rec2_t* rec2, const int32_t* n2, const int64_t* n_steps,
                       const int64_t* n_steps_cumsum, int64_t rec_stride, const int64_t* off3, int64_t n_rays,
                       const float* rays_start, const float* rays_dir, float stepdist,
                       const float* xyz_min, const float* xyz_max, const float* alphainv_last, float interval,
                       const float* rays_o, const float* rays_d, float near, float far,
                       const float* density, int X, int Y, int Z,
                       const float* k0, int C, int64_t sC, int64_t sX, int64_t sY, int64_t sZ,
                       const float* grad_weights, const float* grad_last, const float* grad_feat,
                       float* grad_o, float* grad_d, void* stream) {
  if (n_rays < 0 || C < 0 || X <= 0 || Y <= 0 || Z <= 0 || !(stepdist > 0.0f)) return DVGO_EINVAL;   // NDC spacing is not differentiated
  if (n_rays == 0) return 0;
  if (!rec2 || !n2 || !n_steps || !off3 || !rays_start || !rays_dir || !xyz_min || !xyz_max || !alphainv_last ||
      !rays_o || !rays_d || !density || !grad_o || !grad_d)
    return DVGO_EINVAL;       // grad_weights may be NULL when M3 == 0 (it is only read for flagged samples)
  if (grad_feat && C > 0 && !k0) return DVGO_EINVAL;
  if (!n_steps_cumsum && rec_stride <= 0) return DVGO_EINVAL;
  if (!dvgo_fits(n_rays * 64)) return DVGO_ERANGE;
  const RayGradParams P = ray_grad_params(xyz_min, xyz_max, stepdist, X, Y, Z, interval);
  const bool vec = (sC == 1) && (C % 4 == 0) && (sX % 4 == 0) && (sY % 4 == 0) && (sZ % 4 == 0) &&
                   ((((uintptr_t)k0) & 15) == 0) && ((((uintptr_t)grad_feat) & 15) == 0);
  const int blocks = dvgo_blocks(n_rays * 64, DVGO_BLOCK);
  if (vec)
    march_ray_bwd_kernel<4><<<blocks, DVGO_BLOCK, 0, (hipStream_t)stream>>>(
        rec2, n2, n_steps, n_steps_cumsum, rec_stride, off3, n_rays, rays_start, rays_dir, P, alphainv_last, rays_o, rays_d,
        near, far, density, k0, C, sC, sX, sY, sZ, grad_weights, grad_last, grad_feat, grad_o, grad_d);
  else
    march_ray_bwd_kernel<1><<<blocks, DVGO_BLOCK, 0, (hipStream_t)stream>>>(
        rec2, n2, n_steps, n_steps_cumsum, rec_stride, off3, n_rays, rays_start, rays_dir, P, alphainv_last, rays_o, rays_d,
        near, far, density, k0, C, sC, sX, sY, sZ, grad_weights, grad_last, grad_feat, grad_o, grad_d);
  DVGO_LAUNCH_CHECK();
  return 0;
}

int dvgo_march_ray_bwd_pts(const dvgo_rec2_t* rec2, const int32_t* n2, const int64_t* n_steps,
                           const int64_t* n_steps_cumsum, int64_t rec_stride, const int64_t* off3, int64_t n_rays,
                           const float* rays_start, const float* rays_dir, float stepdist,
                           const float* xyz_min, const float* xyz_max, const float* alphainv_last, float interval,
                           const float* rays_o, const float* rays_d, float near, float far,
                           const float* density, int X, int Y, int Z,
                           const float* grad_weights, const float* grad_last, const float* grad_pts,
                           float* grad_o, float* grad_d, void* stream) {
  if (n_rays < 0 || X <= 0 || Y <= 0 || Z <= 0 || !(stepdist > 0.0f)) return DVGO_EINVAL;   // NDC spacing is not differentiated
  if (n_rays == 0) return 0;
  if (!rec2 || !n2 || !n_steps || !off3 || !rays_start || !rays_dir || !xyz_min || !xyz_max || !alphainv_last ||
      !rays_o || !rays_d || !density || !grad_o || !grad_d)
    return DVGO_EINVAL;       // grad_weights may be NULL when M3 == 0 (it is only read for flagged records), grad_pts: no second term
  if (!n_steps_cumsum && rec_stride <= 0) return DVGO_EINVAL;
  if (!dvgo_fits(n_rays * 64)) return DVGO_ERANGE;
  const RayGradParams P = ray_grad_params(xyz_min, xyz_max, stepdist, X, Y, Z, interval);
  march_pts_ray_bwd_kernel<<<dvgo_blocks(n_rays * 64, DVGO_BLOCK), DVGO_BLOCK, 0, (hipStream_t)stream>>>(
      rec2, n2, n_steps, n_steps_cumsum, rec_stride, off3, n_rays, rays_start, rays_dir, P, alphainv_last, rays_o, rays_d,
      near, far, density, grad_weights, grad_last, grad_pts, grad_o, grad_d);
  DVGO_LAUNCH_CHECK();
  return 0;
}

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
                          int R, const float* grad_weights, const float* grad_last, const float* grad_pts,
                          float* grad_o, float* grad_d, void* stream) {
  const TpPlanes Q = TP_PLANES(xy, yz, zx);
  const VmLines L = VM_LINES();
  // shapes first (dvgo_march_vm_density's order), among them what its march does not do: NDC spacing, the exact record layout
  if (n_rays < 0 || R < 1 || !tp_plane_ok(Q.a) || !tp_plane_ok(Q.b) || !tp_plane_ok(Q.c) || L.a.N < 1 || L.b.N < 1 || L.c.N < 1 ||
      !(stepdist > 0.0f) || rec_stride <= 0)
    return DVGO_EINVAL;
  if (n_rays == 0) return 0;
  if (!rec2 || !n2 || !off3 || !rays_start || !rays_dir || !xyz_min || !xyz_max || !alphainv_last || !rays_o || !rays_d ||
      !Q.a.p || !Q.b.p || !Q.c.p || !L.a.p || !L.b.p || !L.c.p || !grad_o || !grad_d)
    return DVGO_EINVAL;       // grad_weights may be NULL when M3 == 0, grad_last and grad_pts when there is none
  if (!dvgo_fits(n_rays * 64) || !dvgo_fits(rec_stride)) return DVGO_ERANGE;
  const RayGradParams P = ray_grad_params(xyz_min, xyz_max, stepdist, 0, 0, 0, interval);
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (R % 4 == 0) && tp_planes_vec(Q, 4) && vm_line_vec(L.a) && vm_line_vec(L.b) && vm_line_vec(L.c);
  const int blocks = dvgo_blocks(n_rays * 64, DVGO_BLOCK);
  if (vec)
    march_vm_ray_bwd_kernel<4><<<blocks, DVGO_BLOCK, 0, st>>>(Q.a, Q.b, Q.c, L.a, L.b, L.c, R, rec2, n2, rec_stride, off3, n_rays,
                                                              rays_start, rays_dir, P, alphainv_last, rays_o, rays_d, near, far,
                                                              grad_weights, grad_last, grad_pts, grad_o, grad_d);
  else
    march_vm_ray_bwd_kernel<1><<<blocks, DVGO_BLOCK, 0, st>>>(Q.a, Q.b, Q.c, L.a, L.b, L.c, R, rec2, n2, rec_stride, off3, n_rays,
                                                              rays_start, rays_dir, P, alphainv_last, rays_o, rays_d, near, far,
                                                              grad_weights, grad_last, grad_pts, grad_o, grad_d);
  DVGO_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
