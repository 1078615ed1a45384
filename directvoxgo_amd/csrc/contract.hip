// Unbounded scenes: the contracted-space sampler and the distortion loss.
//
// Formulas: DVGO v2 (Sun et al., "Improved Direct Voxel Grid Optimization for Radiance Fields Reconstruction",
// arXiv:2206.05085) for the contraction and the cumulative-distance thinning, Mip-NeRF 360 (Barron et al.,
// CVPR 2022) for the distortion loss in its O(n) per-ray form.  The order of operations below is the contract that
// tests/unbounded_oracle.py restates in float32; the library is built with -ffp-contract=off and HIP's correctly
// rounded fp32 division and square root, so sampler outputs are bit-identical to that oracle.
#include "contract_common.h"      // the ray setup, the point, the segment and the occupancy lookup: shared with march_contract.hip

#define DVGO_CONTRACT_BLOCK 64    // one wave per workgroup: a training batch (8192 rays) spreads over 128 CUs

// One step of the per-ray walk: point, contraction, thinning, occupancy.  Returns whether sample k is kept.
// State carried between steps: the previous contracted point and the accumulated distance.
struct ContractWalk {
  float qx, qy, qz;      // this step's contracted point
  float px_, py_, pz_;   // previous contracted point
  float acc;
};

__device__ __forceinline__ bool contract_step(const ContractRay& R, float t, int k, float b, float one_b, int l2,
                                              float thres, const uint8_t* __restrict__ mask, int mi, int mj, int mk,
                                              const float* __restrict__ msc, const float* __restrict__ msh,
                                              ContractWalk& W) {
  const bool inner = contract_point(R, t, b, one_b, l2, W.qx, W.qy, W.qz);
  bool over = false;
  if (k > 0) {
    W.acc = W.acc + contract_segment(W.qx, W.qy, W.qz, W.px_, W.py_, W.pz_);
    over = W.acc > thres;
    if (over) W.acc = 0.0f;
  }
  W.px_ = W.qx; W.py_ = W.qy; W.pz_ = W.qz;
  bool keep = inner || over;
  if (keep && mask != nullptr)
    keep = contract_occupied(W.qx, W.qy, W.qz, mask, mi, mj, mk, msc[0], msc[1], msc[2], msh[0], msh[1], msh[2]);
  return keep;
}

// Ray per lane.  The thinning is a recurrence with reset (acc += d_k; if acc > thres: keep, acc = 0), which has no
// associative form a wave-wide scan could use, so each lane walks its own ray through all n_max steps.  t_k is the
// same for every lane of a step (scalar loads of the table).  Pass 1 counts, pass 2 recomputes and writes the kept
// samples at the ray's offset: ray-major, step-ascending, the order Alphas2Weights and segment_coo need.
template <bool EMIT>
__global__ void __launch_bounds__(DVGO_CONTRACT_BLOCK)
contract_sample_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d, int64_t n_rays, float cx,
                       float cy, float cz, float rx, float ry, float rz, const float* __restrict__ t_tab, int n_max,
                       float b, int l2, float thres, const uint8_t* __restrict__ mask, int mi, int mj, int mk,
                       const float* __restrict__ msc, const float* __restrict__ msh, int32_t* __restrict__ counts,
                       const int64_t* __restrict__ offsets, float* __restrict__ q, int64_t* __restrict__ ray_id,
                       int64_t* __restrict__ step_id, float* __restrict__ t_out) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rays) return;
  const ContractRay R = contract_ray(rays_o, rays_d, r, cx, cy, cz, rx, ry, rz);
  const float one_b = 1.0f + b;
  ContractWalk W;
  W.px_ = W.py_ = W.pz_ = 0.0f;
  W.acc = 0.0f;
  int64_t o = EMIT ? offsets[r] : 0;
  int32_t c = 0;
  for (int k = 0; k < n_max; ++k) {
    const float t = t_tab[k];
    if (!contract_step(R, t, k, b, one_b, l2, thres, mask, mi, mj, mk, msc, msh, W)) continue;
    if (EMIT) {
      q[3 * o + 0] = W.qx;
      q[3 * o + 1] = W.qy;
      q[3 * o + 2] = W.qz;
      ray_id[o] = r;
      step_id[o] = k;
      t_out[o] = t;
      ++o;
    } else {
      ++c;
    }
  }
  if (!EMIT) counts[r] = c;
}

// ----------------------------------------------------------------------------------
// Distortion loss, value and gradient in one launch.  Ray per lane: the lane finds its segment of the (ray-sorted)
// samples by binary search, sums W and S over it (pass 1), then walks it again with the running prefix sums to write
// dL/dw and its share of the loss (pass 2).  Accumulation in double.  The per-ray losses are summed by a fixed tree
// per workgroup; the last workgroup to finish (integer ticket) sums the workgroup partials in index order, so the value
// does not depend on scheduling.  No float atomics.
// ----------------------------------------------------------------------------------
#define DVGO_DIST_BLOCK 256

__device__ __forceinline__ int64_t dist_lower_bound(const int64_t* __restrict__ ray_id, int64_t m, int64_t r) {
  int64_t lo = 0, hi = m;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (ray_id[mid] < r) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ double dist_block_sum(double v, double* sh) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
#pragma unroll
  for (int d = DVGO_DIST_BLOCK / 2; d > 0; d >>= 1) {
    if (tid < d) sh[tid] = sh[tid] + sh[tid + d];
    __syncthreads();
  }
  const double total = sh[0];
  __syncthreads();
  return total;
}

__global__ void __launch_bounds__(DVGO_DIST_BLOCK)
distortion_kernel(const float* __restrict__ w, const float* __restrict__ s, const int64_t* __restrict__ ray_id,
                  int64_t m, int64_t n_rays, double inv_n, double delta, float* __restrict__ grad,
                  double* __restrict__ partials, unsigned int* __restrict__ ticket, float* __restrict__ loss) {
  __shared__ double sh[DVGO_DIST_BLOCK];
  __shared__ bool last_s;
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double lr = 0.0;
  if (r < n_rays) {
    const int64_t i0 = dist_lower_bound(ray_id, m, r);
    const int64_t i1 = dist_lower_bound(ray_id, m, r + 1);
    double wt = 0.0, st = 0.0;
    for (int64_t i = i0; i < i1; ++i) {
      const double wi = w[i];
      wt += wi;
      st += wi * (double)s[i];
    }
    double wb = 0.0, sb = 0.0, cross = 0.0, self = 0.0;   // W_<i, S_<i
    for (int64_t i = i0; i < i1; ++i) {
      const double wi = w[i], si = s[i];
      const double before = si * wb - sb;
      const double wa = wb + wi, sa = sb + wi * si;      // W_<=i, S_<=i
      const double after = (st - sa) - si * (wt - wa);  // sum_{j>i} w_j (s_j - s_i)
      cross += wi * before;
      self += wi * wi;
      grad[i] = (float)(2.0 * inv_n * (before + after) + (2.0 / 3.0) * delta * wi * inv_n);
      wb = wa;
      sb = sa;
    }
    lr = 2.0 * cross + delta * self / 3.0;
  }
  const double bsum = dist_block_sum(lr, sh);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = bsum;
    __threadfence();
    last_s = atomicAdd(ticket, 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (!last_s) return;
  __threadfence();
  const volatile double* vp = partials;
  double acc = 0.0;
  for (int64_t b = threadIdx.x; b < gridDim.x; b += DVGO_DIST_BLOCK) acc += vp[b];
  const double total = dist_block_sum(acc, sh);
  if (threadIdx.x == 0) *loss = (float)(total * inv_n);
}

// ----------------------------------------------------------------------------------
extern "C" {

int dvgo_contract_count(const float* rays_o, const float* rays_d, int64_t n_rays, const float* center,
                        const float* radius, const float* t_tab, int n_max, float bg_len, int l2, float thres,
                        const uint8_t* mask, int mi, int mj, int mk, const float* mask_scale,
                        const float* mask_shift, int32_t* counts, void* stream) {
  if (n_rays < 0 || n_max < 0 || mi < 0 || mj < 0 || mk < 0) return DVGO_EINVAL;
  if (n_rays == 0) return 0;
  if (!rays_o || !rays_d || !center || !radius || !counts || (n_max > 0 && !t_tab)) return DVGO_EINVAL;
  if (mask && (!mask_scale || !mask_shift)) return DVGO_EINVAL;
  if (!dvgo_fits(n_rays)) return DVGO_ERANGE;
  contract_sample_kernel<false><<<dvgo_blocks(n_rays, DVGO_CONTRACT_BLOCK), DVGO_CONTRACT_BLOCK, 0,
                                  (hipStream_t)stream>>>(
      rays_o, rays_d, n_rays, center[0], center[1], center[2], radius[0], radius[1], radius[2], t_tab, n_max,
      bg_len, l2, thres, mask, mi, mj, mk, mask_scale, mask_shift, counts, nullptr, nullptr, nullptr, nullptr,
      nullptr);
  DVGO_LAUNCH_CHECK();
  return 0;
}

int dvgo_contract_emit(const float* rays_o, const float* rays_d, int64_t n_rays, const float* center,
                       const float* radius, const float* t_tab, int n_max, float bg_len, int l2, float thres,
                       const uint8_t* mask, int mi, int mj, int mk, const float* mask_scale, const float* mask_shift,
                       const int64_t* offsets, float* q, int64_t* ray_id, int64_t* step_id, float* t,
                       void* stream) {
  if (n_rays < 0 || n_max < 0 || mi < 0 || mj < 0 || mk < 0) return DVGO_EINVAL;
  if (n_rays == 0) return 0;
  if (!rays_o || !rays_d || !center || !radius || !offsets || !q || !ray_id || !step_id || !t ||
      (n_max > 0 && !t_tab))
    return DVGO_EINVAL;
  if (mask && (!mask_scale || !mask_shift)) return DVGO_EINVAL;
  if (!dvgo_fits(n_rays)) return DVGO_ERANGE;
  contract_sample_kernel<true><<<dvgo_blocks(n_rays, DVGO_CONTRACT_BLOCK), DVGO_CONTRACT_BLOCK, 0,
                                 (hipStream_t)stream>>>(
      rays_o, rays_d, n_rays, center[0], center[1], center[2], radius[0], radius[1], radius[2], t_tab, n_max,
      bg_len, l2, thres, mask, mi, mj, mk, mask_scale, mask_shift, nullptr, offsets, q, ray_id, step_id, t);
  DVGO_LAUNCH_CHECK();
  return 0;
}

int dvgo_distortion_fwd_bwd(const float* w, const float* s, const int64_t* ray_id, int64_t m, int64_t n_rays,
                            int64_t n_norm, int n_max, float* grad, double* partials, unsigned int* ticket,
                            float* loss, void* stream) {
  if (m < 0 || n_rays < 0 || n_norm <= 0 || n_max <= 0) return DVGO_EINVAL;
  if (!loss || !ticket || (n_rays > 0 && !partials) || (m > 0 && (!w || !s || !ray_id || !grad))) return DVGO_EINVAL;
  if (n_rays == 0) {
    DVGO_HIP_TRY(hipMemsetAsync(loss, 0, sizeof(float), (hipStream_t)stream));
    return 0;
  }
  if (!dvgo_fits(n_rays) || !dvgo_fits(m)) return DVGO_ERANGE;
  distortion_kernel<<<dvgo_blocks(n_rays, DVGO_DIST_BLOCK), DVGO_DIST_BLOCK, 0, (hipStream_t)stream>>>(
      w, s, ray_id, m, n_rays, 1.0 / (double)n_norm, 1.0 / (double)n_max, grad, partials, ticket, loss);
  DVGO_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
