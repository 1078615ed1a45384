// What the fused marches share (march.hip: the dense grid; march_vm.hip: the decomposed density; march_contract.hip: the
// contracted space; march_raygrad.hip and contract_raygrad.hip: their ray gradients), each piece stated once so that all
// form the same bits by construction: the lane mask, the wave sum, the suffix sum and where a ray's records start; forward, the activation (e and alpha), the plain transmittance walk and the commit of a chunk into
// the ray's rec2 records; backward, one chunk of the walk over those records from the far end, and on top of it the walk
// that leaves one raw-density gradient and one position per record and scatters nothing.  The occupancy lookup is
// common.h's dvgo_mask_index.  Everything here must be called by all 64 lanes.
#pragma once
#include "common.h"

__device__ __forceinline__ unsigned long long lanemask_lt(int lane) {
  return (lane == 0) ? 0ull : (~0ull >> (64 - lane));
}

// the sum of v over the 64 lanes, in every lane: a butterfly, so the order is fixed
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// Scratch records of ray r start at cum[r]-n_steps[r] (exact, ray-major M0 layout) when the
// inclusive cumsum is given, else at r*rec_stride (fixed stride = an upper bound of n_steps,
// which saves the scan and the host read of M0).
__device__ __forceinline__ int64_t rec_base(const int64_t* __restrict__ cum, const int64_t* __restrict__ n_steps,
                                            int64_t rec_stride, int64_t ray) {
  return cum ? (cum[ray] - n_steps[ray]) : ray * rec_stride;
}

// exclusive suffix sum across the wave: sum of v over lanes > lane
__device__ __forceinline__ float wave_suffix_excl(float v, int lane, float& total) {
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

// Raw density d -> e = exp(d + shift) and alpha = 1 - (1 + e)^-interval (K9).  The alpha filter that follows it in every
// march (the reference's first threshold, before transmittance: `if (filt) keep = a > thres`) is one compare and stays at
// the call: march.hip's DVGO_TUNE_EXPERIMENT branch forms e and a another way and joins in front of it.
__device__ __forceinline__ void march_alpha(float d, float act_shift, float interval, float& e, float& a) {
  e = expf(d + act_shift);
  a = 1.0f - dvgo_pow_neg(1.0f + e, -interval);
}

// The transmittance walk of one 64-step chunk in the reference's order and precision (K12, render_utils_kernel.cu:448-454):
//   T_cum = (float)((double)T_cum * (1. - alpha + 1e-10)), stop after the first sample with (double)T_cum < 1e-3.
// `todo`: kept lanes (wave-uniform; a dropped sample never enters compositing), `f`: per-lane double factor
// 1 - alpha + 1e-10.  Each step is one exec-masked multiply on lane j and a v_readlane of the result, so T, the weights and
// every threshold decision are bit-identical to the serial code.  Returns the lane that stopped the ray or -1.
// (march.hip: chain_walk is the same walk hand-scheduled.)
__device__ __forceinline__ int plain_walk(unsigned long long todo, double f, int lane, float& Tc, float& T_before) {
  int stop_lane = -1;
  while (todo) {
    const int j = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    float T_after = 1.0f;
    if (lane == j) { T_before = Tc; T_after = (float)((double)Tc * f); }
    Tc = dvgo_readlane_f(T_after, j);
    // (double)T < 1e-3  <=>  T < 1e-3f for floats (1e-3f is the float just above the double 1e-3); T >= 0 (or NaN, which
    // does not stop), so the ordered-unsigned compare of the bit patterns is the same test and stays on the scalar unit
    if (__float_as_uint(Tc) < 0x3A83126Fu) { stop_lane = j; break; }
  }
  return stop_lane;
}

// What a chunk leaves behind its walk: the cut at the stop lane, the weight filter (w = T_before * alpha > thres) and the
// ballot / popcount compaction of the surviving lanes into the ray's records from rec2[cs0 + c2] on, "kept" in bit 31 of
// the step; c2 / c3 count the records / the kept ones.  The counts go in and come back by value: a count passed by
// reference is promoted to a register a pass later than the kernel's other loop variables, and that alone changed the
// kernels' register allocation (spills, instruction order).
struct MarchCommit {
  bool valid2;      // this lane wrote a record
  int c2, c3;       // the ray's records / kept records, this chunk included
};

__device__ __forceinline__ MarchCommit march_commit(bool keep, int stop_lane, int step, float e, float a, float T_before,
                                                    bool filt, float thres, int lane, unsigned long long lt,
                                                    dvgo_rec2_t* rec2, int64_t cs0, int c2, int c3) {
  MarchCommit cm;
  const bool valid2 = keep && (stop_lane < 0 || lane <= stop_lane);
  const float w = T_before * a;
  const bool keep3 = valid2 && (!filt || (w > thres));
  const unsigned long long m2 = __ballot(valid2), m3 = __ballot(keep3);
  if (valid2) {
    dvgo_rec2_t r;
    r.step = step | (keep3 ? (int32_t)0x80000000 : 0);
    r.exp_d = e; r.alpha = a; r.T = T_before;
    rec2[cs0 + c2 + __popcll(m2 & lt)] = r;
  }
  cm.valid2 = valid2;
  cm.c2 = c2 + __popcll(m2);
  cm.c3 = c3 + __popcll(m3);
  return cm;
}

// One chunk of the backward walk: the records [cs0 + lo, cs0 + lo + n) of a ray, n <= 64, chunks taken from the far end.
//   K13 (render_utils_kernel.cu:521-530): g_alpha = g_w*T - acc/((1-alpha)+1e-10), acc += g_w*w
//   K10 (:402-405) raw2alpha backward: g_d, the gradient of the record's raw density
// `c3_rem` (kept records not yet visited) and `acc` are carried from chunk to chunk.  A kept record (`flag`) is number
// `rank` of the ray's kept samples, grad_weights[o3 + rank] its weight gradient.  march_bwd_chunk does what all 64 lanes
// take part in (the ballot, the suffix sum); g_d() finishes a lane that has a record (`act`), and the caller invokes it
// inside the one `if (act)` block that also forms the record's position: the kernels keep a single divergent region.
struct MarchBwdChunk {
  bool act, flag;
  int step, rank;
  dvgo_rec2_t rec;
  float gw, my_acc;     // the record's weight gradient (0 unless kept); acc behind this lane
  __device__ __forceinline__ float g_d(float interval) const {
    const float gt = gw * rec.T;
    const float one_minus = 1.0f - rec.alpha;
    const float g_alpha = (float)((double)gt - (double)my_acc / ((double)one_minus + 1e-10));
    double v = fmin((double)rec.exp_d, 1e10) * (double)dvgo_pow_neg(1.0f + rec.exp_d, -interval - 1.0f);
    v = v * (double)interval;
    v = v * (double)g_alpha;
    return (float)v;
  }
};

__device__ __forceinline__ MarchBwdChunk march_bwd_chunk(const dvgo_rec2_t* __restrict__ rec2, int64_t cs0, int lo, int n,
                                                         int lane, unsigned long long lt, int64_t o3, int& c3_rem,
                                                         float& acc, const float* __restrict__ grad_weights) {
  MarchBwdChunk k;
  k.act = lane < n;
  dvgo_rec2_t rec;
  rec.step = 0; rec.exp_d = 0.f; rec.alpha = 0.f; rec.T = 0.f;
  if (k.act) rec = rec2[cs0 + lo + lane];
  k.flag = k.act && (rec.step < 0);
  k.step = rec.step & 0x7fffffff;
  const unsigned long long m = __ballot(k.flag);
  const int cnt = __popcll(m);
  k.rank = c3_rem - cnt + __popcll(m & lt);
  c3_rem -= cnt;
  const float gw = k.flag ? grad_weights[o3 + k.rank] : 0.0f;
  const float w = rec.T * rec.alpha;
  float total;
  const float suffix = wave_suffix_excl(gw * w, lane, total);   // inactive lanes contribute 0
  k.rec = rec; k.gw = gw;
  k.my_acc = acc + suffix;
  acc += total;
  return k;
}

// One wavefront over the records [cs0, cs0 + c2) of ray `ray` from the far end.  Record i writes g_raw[o2 + i] and its
// position, which `pos(step, x, y, z)` forms, at xyz2[o2 + i].  c2 is wave-uniform.
template <class Pos>
__device__ __forceinline__ void march_records_bwd(const dvgo_rec2_t* __restrict__ rec2, int c2, int64_t cs0, int64_t o3,
                                                  int c3_rem, int64_t o2, int lane, float acc, float interval,
                                                  const float* __restrict__ grad_weights, float* __restrict__ g_raw,
                                                  float* __restrict__ xyz2, Pos pos) {
  const unsigned long long lt = lanemask_lt(lane);
  for (int hi = c2; hi > 0; hi -= 64) {
    const int lo = max(0, hi - 64);
    const MarchBwdChunk k = march_bwd_chunk(rec2, cs0, lo, hi - lo, lane, lt, o3, c3_rem, acc, grad_weights);
    if (k.act) {
      const float g_d = k.g_d(interval);
      const int64_t i = o2 + lo + lane;
      g_raw[i] = g_d;
      float x, y, z;
      pos(k.step, x, y, z);
      xyz2[3 * i] = x; xyz2[3 * i + 1] = y; xyz2[3 * i + 2] = z;
    }
  }
}
