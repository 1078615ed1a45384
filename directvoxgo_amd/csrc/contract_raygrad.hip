// Ray gradients through the scene contraction: given dL/dq for the kept
// samples of DirectContractedVoxGO, the gradient of the rays they lie on.  include/dvgo_hip.h (the contraction's ray
// gradient block) is the contract, tests/contract_raygrad_oracle.py restates it in float64.
//
//   contract_ray_bwd_kernel<false>   the samples are a ray-major list: rows off[r] .. off[r + 1] of grad_q / step_id
//   contract_ray_bwd_kernel<true>    the samples are the fused march's records: record i of ray r is rec2[r * rec_stride + i],
//                                    its gradient row off2[r] + i
//
// One wavefront per ray, lanes = 64 consecutive samples per chunk, chunks ascending.  A lane rebuilds p and n of its
// sample from the ray and the table (contract_common.h: the forward's bits, so the inner test and the arg-max axis are the
// forward's), applies the contraction's Jacobian to its row of grad_q and adds the result, and t times the result, to six
// float32 accumulators that live across chunks.  One butterfly over the 64 lanes at the end; lane 0 applies the ray's own
// Jacobian (the normalisation of d included) and writes grad_o / grad_d with plain stores.  A lane's row of grad_q is 12
// contiguous bytes and the 64 rows of a chunk are 768 contiguous bytes.  No atomics, no LDS, no workspace, nothing to zero
// beforehand: bitwise repeatable.
#include "contract_common.h"
#include "march_records.h"      // wave_sum

struct ContractRayBwdParams {
  float cx, cy, cz, rx, ry, rz;   // centre and radius of the foreground box
  float b;                        // bg_len
  int l2;
};

// g_p = J^T g for one sample: g if n <= 1, else f(n) g + w f'(n) (p . g) with w = p / n ('l2') or sign(p_a) e_a, a the lowest
// axis attaining max|p_a| ('inf').  g == 0 gives exact zeros.
__device__ __forceinline__ void contract_point_bwd(const ContractRay& R, float t, float b, float one_b, int l2, float gx,
                                                   float gy, float gz, float& hx, float& hy, float& hz) {
  float px, py, pz;
  const float n = contract_norm(R, t, l2, px, py, pz);
  if (n <= 1.0f) {
    hx = gx; hy = gy; hz = gz;
    return;
  }
  const float f = (one_b - b / n) / n;
  const float fp = ((2.0f * b) / n - one_b) / (n * n);
  const float c = fp * ((px * gx + py * gy) + pz * gz);
  hx = f * gx; hy = f * gy; hz = f * gz;
  if (l2) {
    hx = hx + (px / n) * c;
    hy = hy + (py / n) * c;
    hz = hz + (pz / n) * c;
  } else {
    const float ax = fabsf(px), ay = fabsf(py), az = fabsf(pz);
    if (ax >= ay && ax >= az) hx = hx + (px < 0.0f ? -c : c);
    else if (ay >= az)        hy = hy + (py < 0.0f ? -c : c);
    else                      hz = hz + (pz < 0.0f ? -c : c);
  }
}

__device__ __forceinline__ int64_t crb_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <bool REC>
__global__ void __launch_bounds__(DVGO_BLOCK)
contract_ray_bwd_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d, int64_t n_rays,
                        const float* __restrict__ t_tab, int n_max, ContractRayBwdParams P,
                        const float* __restrict__ grad_q, int64_t M, const int64_t* __restrict__ step_id,
                        const int64_t* __restrict__ off, const dvgo_rec2_t* __restrict__ rec2,
                        const int32_t* __restrict__ n2, int64_t rec_stride, float* __restrict__ grad_o,
                        float* __restrict__ grad_d) {
  const int64_t ray = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (ray >= n_rays) return;
  // rows [g0, g0 + cnt) of grad_q; nothing outside [0, M) is read: a list that runs past it is cut there (REC: flagged)
  int64_t g0 = off[ray], cnt;
  bool bad = false;
  if (REC) {
    cnt = crb_clamp(n2[ray], 0, rec_stride);
    if (cnt > 0 && (g0 < 0 || g0 + cnt > M)) { bad = true; cnt = 0; }
  } else {
    g0 = crb_clamp(g0, 0, M);
    cnt = crb_clamp(off[ray + 1], g0, M) - g0;
  }
  if (cnt == 0 && !bad) {                          // a ray without samples: exact zeros, whatever its direction
    if (lane < 3) { grad_o[3 * ray + lane] = 0.0f; grad_d[3 * ray + lane] = 0.0f; }
    return;
  }
  float nu;
  const ContractRay R = contract_ray(rays_o, rays_d, ray, P.cx, P.cy, P.cz, P.rx, P.ry, P.rz, nu);
  const float one_b = 1.0f + P.b;
  const int64_t cs0 = ray * rec_stride;
  float Ax = 0.f, Ay = 0.f, Az = 0.f, Bx = 0.f, By = 0.f, Bz = 0.f;
  for (int64_t base = 0; base < cnt; base += 64) {
    const int64_t i = base + lane;
    if (i >= cnt) continue;
    const int64_t k = REC ? (int64_t)(rec2[cs0 + i].step & 0x7fffffff) : step_id[g0 + i];
    if (k < 0 || k >= n_max) { bad = true; continue; }
    const float* g = grad_q + 3 * (g0 + i);
    const float gx = g[0], gy = g[1], gz = g[2];
    const float t = t_tab[k];
    float hx, hy, hz;
    contract_point_bwd(R, t, P.b, one_b, P.l2, gx, gy, gz, hx, hy, hz);
    Ax = Ax + hx; Ay = Ay + hy; Az = Az + hz;
    Bx = Bx + t * hx; By = By + t * hy; Bz = Bz + t * hz;
  }
  Ax = wave_sum(Ax); Ay = wave_sum(Ay); Az = wave_sum(Az);
  Bx = wave_sum(Bx); By = wave_sum(By); Bz = wave_sum(Bz);
  const bool any_bad = __ballot(bad) != 0ull;
  if (lane != 0) return;
  float ox = Ax / P.rx, oy = Ay / P.ry, oz = Az / P.rz;
  const float dB = (R.dx * Bx + R.dy * By) + R.dz * Bz;
  float dx = ((Bx - R.dx * dB) / nu) / P.rx;
  float dy = ((By - R.dy * dB) / nu) / P.ry;
  float dz = ((Bz - R.dz * dB) / nu) / P.rz;
  if (any_bad) ox = oy = oz = dx = dy = dz = __int_as_float(0x7fc00000);   // a step outside the table: the ray says so
  grad_o[3 * ray] = ox; grad_o[3 * ray + 1] = oy; grad_o[3 * ray + 2] = oz;
  grad_d[3 * ray] = dx; grad_d[3 * ray + 1] = dy; grad_d[3 * ray + 2] = dz;
}

static ContractRayBwdParams crb_params(const float* center, const float* radius, float bg_len, int l2) {
  ContractRayBwdParams P = {};
  P.cx = center[0]; P.cy = center[1]; P.cz = center[2];
  P.rx = radius[0]; P.ry = radius[1]; P.rz = radius[2];
  P.b = bg_len; P.l2 = l2;
  return P;
}

extern "C" {

// NOTE: center / radius are HOST pointers (3 floats each), as in march_contract.hip's entries.

int dvgo_contract_ray_bwd(const float* rays_o, const float* rays_d, int64_t n_rays, const float* center,
                          const float* radius, const float* t_tab, int n_max, float bg_len, int l2, const float* grad_q,
                          const int64_t* step_id, int64_t M, const int64_t* off, float* grad_o, float* grad_d,
                          void* stream) {
  if (n_rays < 0 || M < 0 || n_max <= 0) return DVGO_EINVAL;
  if (n_rays == 0) return 0;
  if (!rays_o || !rays_d || !center || !radius || !t_tab || !off || !grad_o || !grad_d) return DVGO_EINVAL;
  if (M > 0 && (!grad_q || !step_id)) return DVGO_EINVAL;
  if (!dvgo_fits(n_rays * 64)) return DVGO_ERANGE;
  contract_ray_bwd_kernel<false><<<dvgo_blocks(n_rays * 64, DVGO_BLOCK), DVGO_BLOCK, 0, (hipStream_t)stream>>>(
      rays_o, rays_d, n_rays, t_tab, n_max, crb_params(center, radius, bg_len, l2), grad_q, M, step_id, off, nullptr,
      nullptr, 0, grad_o, grad_d);
  DVGO_LAUNCH_CHECK();
  return 0;
}

int dvgo_contract_ray_bwd_rec(const float* rays_o, const float* rays_d, int64_t n_rays, const float* center,
                              const float* radius, const float* t_tab, int n_max, float bg_len, int l2,
                              const dvgo_rec2_t* rec2, const int32_t* n2, int64_t rec_stride, const int64_t* off2,
                              const float* grad_q2, int64_t M2, float* grad_o, float* grad_d, void* stream) {
  if (n_rays < 0 || M2 < 0 || n_max <= 0 || rec_stride < 0) return DVGO_EINVAL;
  if (n_rays == 0) return 0;
  if (!rays_o || !rays_d || !center || !radius || !t_tab || !n2 || !off2 || !grad_o || !grad_d) return DVGO_EINVAL;
  if (M2 > 0 && (!grad_q2 || !rec2)) return DVGO_EINVAL;
  if (!dvgo_fits(n_rays * 64) || !dvgo_fits(rec_stride)) return DVGO_ERANGE;
  contract_ray_bwd_kernel<true><<<dvgo_blocks(n_rays * 64, DVGO_BLOCK), DVGO_BLOCK, 0, (hipStream_t)stream>>>(
      rays_o, rays_d, n_rays, t_tab, n_max, crb_params(center, radius, bg_len, l2), grad_q2, M2, nullptr, off2, rec2, n2,
      rec_stride, grad_o, grad_d);
  DVGO_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
