// What the record-per-gradient marches share (march_vm.hip: the decomposed density; march_contract.hip: the contracted
// space): the lane mask, the suffix sum and the backward walk over a ray's rec2 records, which leaves one raw-density
// gradient and one position per record and scatters nothing.  The walk is march.hip's march_density_bwd_kernel, expression
// for expression (include/dvgo_hip.h, dvgo_march_vm_density_bwd, states it); only where a record's position comes from
// differs between the two callers.
#pragma once
#include "common.h"

__device__ __forceinline__ unsigned long long mvm_lanemask_lt(int lane) {
  return (lane == 0) ? 0ull : (~0ull >> (64 - lane));
}

// exclusive suffix sum across the wave: sum of v over lanes > lane (march.hip: wave_suffix_excl, the same shuffles and adds)
__device__ __forceinline__ float mvm_suffix_excl(float v, int lane, float& total) {
  float inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float o = __shfl_down(inc, d);
    if (lane + d < 64) inc += o;
  }
  total = dvgo_readlane_f(inc, 0);
  float ex = __shfl_down(inc, 1);
  if (lane == 63) ex = 0.0f;
  return ex;
}

// One wavefront over the records [cs0, cs0 + c2) of ray `ray` from the far end.  Record i writes g_raw[o2 + i] and its
// position, which `pos(step, x, y, z)` forms, at xyz2[o2 + i].  Must be called by all 64 lanes; c2 is wave-uniform.
template <class Pos>
__device__ __forceinline__ void march_records_bwd(const dvgo_rec2_t* __restrict__ rec2, int c2, int64_t cs0, int64_t o3,
                                                  int c3_rem, int64_t o2, int lane, float acc, float interval,
                                                  const float* __restrict__ grad_weights, float* __restrict__ g_raw,
                                                  float* __restrict__ xyz2, Pos pos) {
  const unsigned long long lt = mvm_lanemask_lt(lane);
  for (int hi = c2; hi > 0; hi -= 64) {
    const int lo = max(0, hi - 64);
    const int n = hi - lo;
    const bool act = lane < n;
    dvgo_rec2_t rec;
    rec.step = 0; rec.exp_d = 0.f; rec.alpha = 0.f; rec.T = 0.f;
    if (act) rec = rec2[cs0 + lo + lane];
    const bool flag = act && (rec.step < 0);
    const int step = rec.step & 0x7fffffff;
    const unsigned long long m = __ballot(flag);
    const int cnt = __popcll(m);
    const int rank = c3_rem - cnt + __popcll(m & lt);
    c3_rem -= cnt;
    const float gw = flag ? grad_weights[o3 + rank] : 0.0f;
    const float w = rec.T * rec.alpha;
    float total;
    const float suffix = mvm_suffix_excl(gw * w, lane, total);   // inactive lanes contribute 0
    const float my_acc = acc + suffix;
    acc += total;
    if (act) {
      const float gt = gw * rec.T;
      const float one_minus = 1.0f - rec.alpha;
      const float g_alpha = (float)((double)gt - (double)my_acc / ((double)one_minus + 1e-10));
      double v = fmin((double)rec.exp_d, 1e10) * (double)dvgo_pow_neg(1.0f + rec.exp_d, -interval - 1.0f);
      v = v * (double)interval;
      v = v * (double)g_alpha;
      const int64_t i = o2 + lo + lane;
      g_raw[i] = (float)v;
      float x, y, z;
      pos(step, x, y, z);
      xyz2[3 * i] = x; xyz2[3 * i + 1] = y; xyz2[3 * i + 2] = z;
    }
  }
}
