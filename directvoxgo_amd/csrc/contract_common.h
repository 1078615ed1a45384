// What the translation units of the contracted space share (contract.hip: the ray-per-lane sampler; march_contract.hip:
// the fused march, step per lane; contract_raygrad.hip: the ray gradient): the ray setup, the point and its contraction, the segment length of the thinning and the
// occupancy lookup.  One set of float32 expressions, so that all kernels form the same bits; the library is built with
// -ffp-contract=off and correctly rounded division and square root.  include/dvgo_hip.h (the unbounded-scenes block) states
// the arithmetic, tests/unbounded_oracle.py restates it.
#pragma once
#include "common.h"

struct ContractRay {
  float ox, oy, oz, dx, dy, dz;
};

// o' = (o - c) / r ; u = d / r ; d' = u / ||u||_2.  `nu` receives ||u||_2 (contract_raygrad.hip: the ray Jacobian divides by it).
__device__ __forceinline__ ContractRay contract_ray(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                    int64_t r, float cx, float cy, float cz, float rx, float ry,
                                                    float rz, float& nu) {
  ContractRay R;
  R.ox = (rays_o[3 * r + 0] - cx) / rx;
  R.oy = (rays_o[3 * r + 1] - cy) / ry;
  R.oz = (rays_o[3 * r + 2] - cz) / rz;
  const float ux = rays_d[3 * r + 0] / rx, uy = rays_d[3 * r + 1] / ry, uz = rays_d[3 * r + 2] / rz;
  nu = sqrtf(ux * ux + uy * uy + uz * uz);
  R.dx = ux / nu;
  R.dy = uy / nu;
  R.dz = uz / nu;
  return R;
}

__device__ __forceinline__ ContractRay contract_ray(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                    int64_t r, float cx, float cy, float cz, float rx, float ry,
                                                    float rz) {
  float nu;
  return contract_ray(rays_o, rays_d, r, cx, cy, cz, rx, ry, rz, nu);
}

// p = o' + d' * t and its norm n = max|p| or ||p||_2: the first half of contract_point, which contract_raygrad.hip
// differentiates at the same bits
__device__ __forceinline__ float contract_norm(const ContractRay& R, float t, int l2, float& px, float& py, float& pz) {
  px = R.ox + R.dx * t; py = R.oy + R.dy * t; pz = R.oz + R.dz * t;
  return l2 ? sqrtf(px * px + py * py + pz * pz) : fmaxf(fmaxf(fabsf(px), fabsf(py)), fabsf(pz));
}

// p = o' + d' * t, n = max|p| or ||p||_2, q = p if n <= 1 else p / n * ((1 + b) - b / n).  Returns n <= 1.
__device__ __forceinline__ bool contract_point(const ContractRay& R, float t, float b, float one_b, int l2, float& qx,
                                               float& qy, float& qz) {
  float px, py, pz;
  const float n = contract_norm(R, t, l2, px, py, pz);
  const bool inner = n <= 1.0f;
  if (inner) {
    qx = px; qy = py; qz = pz;
  } else {
    const float s = one_b - b / n;
    qx = (px / n) * s; qy = (py / n) * s; qz = (pz / n) * s;
  }
  return inner;
}

// ||q - q_prev||_2: what one step adds to the accumulated distance of the thinning
__device__ __forceinline__ float contract_segment(float qx, float qy, float qz, float px_, float py_, float pz_) {
  const float ex = qx - px_, ey = qy - py_, ez = qz - pz_;
  return sqrtf(ex * ex + ey * ey + ez * ez);
}

// MaskCache lookup at q, as maskcache_lookup_kernel computes it
__device__ __forceinline__ bool contract_occupied(float qx, float qy, float qz, const uint8_t* __restrict__ mask, int mi,
                                                  int mj, int mk, float scx, float scy, float scz, float shx, float shy,
                                                  float shz) {
  int64_t idx;
  return dvgo_mask_index(qx, qy, qz, scx, scy, scz, shx, shy, shz, mi, mj, mk, idx) && mask[idx] != 0;
}
