// Tri-plane features: three 2-D feature planes sampled bilinearly at two of a sample's three coordinates, the results
// concatenated or summed, and the gradient scatter into the planes.  Replaces lib/tri_dvgo.py:456-469 grid_sampler2D
// (three F.grid_sample(mode='bilinear', align_corners=True, zero padding) calls, the transposes, torch.cat or +) and
// its autograd backward w.r.t. the planes.
//
// Axes (include/dvgo_hip.h has the table): the reference's ind_norm is the flipped triple and grid_sample's first
// grid component addresses W, so plane xy has rows along y and columns along z, yz rows x / columns y, zx rows z /
// columns x.
//
// Forward: bound by its output write ([M, 3C] floats: 384 B per sample at C = 32 against 12 B of position read and
// planes of a few MB that stay in L2).  A lane owns VEC consecutive channels of one output row -- (sample, plane,
// channel group) for concat, (sample, channel group) for sum -- so a wave's stores are 64 consecutive 16-byte pieces
// of `out`, and in the channels-last layout a texel's channels arrive as 16-byte loads.  The four corner loads are
// unconditional (out-of-range corners read a clamped, valid address and are dropped by a select), so they are in
// flight together; the fma chain then runs in the stated corner order: same bits as skipping.
// VEC = 1 is the same kernel per channel: C % 4 != 0, unaligned bases, channel-first planes.
//
// Backward: 12 C float atomics per sample.  A lane owns (a run of consecutive samples, plane, channel) and keeps the
// four corner sums of the texel cell it is in in registers; it issues its atomics when the cell changes and at the
// end of its run.  Consecutive kept samples of a ray are half a voxel apart, so a cell holds two or three of them.
// Lane order: channel fastest when every plane is channels-last (a wave-instruction adds runs of 4 C contiguous
// bytes), sample fastest otherwise (a wave-instruction adds into neighbouring texels of one channel's plane).
#include "common.h"
#include "plane2d.h"

// total = M * (SUM ? C : 3C) / VEC lanes (< 2^31: the entry checks M * 3C)
template <int VEC, bool SUM>
__global__ void __launch_bounds__(DVGO_BLOCK)
triplane_fwd_kernel(TpPlane PA, TpPlane PB, TpPlane PC, int C, const float* __restrict__ xyz, const float* __restrict__ mn,
                    const float* __restrict__ mx, unsigned int total, float* __restrict__ out) {
  const unsigned int tid = blockIdx.x * (unsigned int)DVGO_BLOCK + threadIdx.x;
  if (tid >= total) return;
  const unsigned int cg = (unsigned int)C / VEC;         // channel groups of a plane
  const unsigned int per = SUM ? cg : 3u * cg;           // lanes of a sample
  const unsigned int m = tid / per, j = tid - m * per;
  TpVal<VEC> r;
  int ah, aw;
  if (SUM) {
    const int c = (int)j * VEC;
    TpPlane q = tp_pick(PA, PB, PC, 0, ah, aw);
    const TpVal<VEC> a = tp_sample<VEC>(q, ah, aw, c, xyz, mn, mx, m);
    q = tp_pick(PA, PB, PC, 1, ah, aw);
    const TpVal<VEC> b = tp_sample<VEC>(q, ah, aw, c, xyz, mn, mx, m);
    q = tp_pick(PA, PB, PC, 2, ah, aw);
    const TpVal<VEC> d = tp_sample<VEC>(q, ah, aw, c, xyz, mn, mx, m);
#pragma unroll
    for (int i = 0; i < VEC; ++i) r.v[i] = (a.v[i] + b.v[i]) + d.v[i];
  } else {
    const unsigned int s = j / cg;
    const int c = (int)(j - s * cg) * VEC;
    const TpPlane q = tp_pick(PA, PB, PC, (int)s, ah, aw);
    r = tp_sample<VEC>(q, ah, aw, c, xyz, mn, mx, m);
  }
  tp_store<VEC>(out + (int64_t)tid * VEC, r);
}

// total = nchunk * 3C lanes, nchunk = ceil(M / run).  CFAST: channel fastest (channels-last planes), else sample fastest.
// The walk is plane2d.h's; plane s reads grad_out[m, s * C + c], or [m, c] when the three are summed.
template <bool CFAST>
__global__ void __launch_bounds__(DVGO_BLOCK)
triplane_bwd_kernel(TpPlane PA, TpPlane PB, TpPlane PC, int C, const float* __restrict__ grad_out, int gstride, int sum,
                    const float* __restrict__ xyz, const float* __restrict__ mn, const float* __restrict__ mx,
                    int64_t M, int run, int64_t nchunk, int64_t total) {
  tp_scatter_lane<CFAST>(PA, PB, PC, C, grad_out, gstride, sum ? 0 : C, xyz, mn, mx, M, run, nchunk, total);
}

extern "C" {

int dvgo_triplane_fwd(const float* xy, int H_xy, int W_xy, int64_t sC_xy, int64_t sH_xy, int64_t sW_xy,
                      const float* yz, int H_yz, int W_yz, int64_t sC_yz, int64_t sH_yz, int64_t sW_yz,
                      const float* zx, int H_zx, int W_zx, int64_t sC_zx, int64_t sH_zx, int64_t sW_zx,
                      int C, const float* xyz, const float* xyz_min, const float* xyz_max, int64_t M, int sum,
                      float* out, void* stream) {
  const TpPlanes P = TP_PLANES(xy, yz, zx);
  const int rc = tp_check(P, C, M, true, xyz, xyz_min, xyz_max, {out}, 3, C);
  if (rc) return rc < 0 ? rc : 0;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (C % 4 == 0) && tp_planes_vec(P, 4) && ((((uintptr_t)out) & 15) == 0);
  const int64_t width = sum ? C : 3 * (int64_t)C;
  const unsigned int total = (unsigned int)(M * width / (vec ? 4 : 1));
  const int blocks = dvgo_blocks(total, DVGO_BLOCK);
  if (vec && sum)
    triplane_fwd_kernel<4, true><<<blocks, DVGO_BLOCK, 0, st>>>(P.a, P.b, P.c, C, xyz, xyz_min, xyz_max, total, out);
  else if (vec)
    triplane_fwd_kernel<4, false><<<blocks, DVGO_BLOCK, 0, st>>>(P.a, P.b, P.c, C, xyz, xyz_min, xyz_max, total, out);
  else if (sum)
    triplane_fwd_kernel<1, true><<<blocks, DVGO_BLOCK, 0, st>>>(P.a, P.b, P.c, C, xyz, xyz_min, xyz_max, total, out);
  else
    triplane_fwd_kernel<1, false><<<blocks, DVGO_BLOCK, 0, st>>>(P.a, P.b, P.c, C, xyz, xyz_min, xyz_max, total, out);
  DVGO_LAUNCH_CHECK();
  return 0;
}

int dvgo_triplane_bwd(const float* grad_out,
                      float* g_xy, int H_xy, int W_xy, int64_t sC_xy, int64_t sH_xy, int64_t sW_xy,
                      float* g_yz, int H_yz, int W_yz, int64_t sC_yz, int64_t sH_yz, int64_t sW_yz,
                      float* g_zx, int H_zx, int W_zx, int64_t sC_zx, int64_t sH_zx, int64_t sW_zx,
                      int C, const float* xyz, const float* xyz_min, const float* xyz_max, int64_t M, int sum,
                      int run, void* stream) {
  const TpPlanes P = TP_PLANES(g_xy, g_yz, g_zx);
  if (run < 0) return DVGO_EINVAL;
  const int rc = tp_check(P, C, M, true, xyz, xyz_min, xyz_max, {grad_out}, 3, C);
  if (rc) return rc < 0 ? rc : 0;
  hipStream_t st = (hipStream_t)stream;
  const TpScatter S = tp_scatter(P, C, M, run, TP_RUN_DEFAULT, 3 * C);
  const int blocks = dvgo_blocks(S.lanes, DVGO_BLOCK);
  const int gstride = sum ? C : 3 * C;
  if (S.cfast)
    triplane_bwd_kernel<true><<<blocks, DVGO_BLOCK, 0, st>>>(P.a, P.b, P.c, C, grad_out, gstride, sum, xyz, xyz_min, xyz_max, M, S.run,
                                                             S.nchunk, S.lanes);
  else
    triplane_bwd_kernel<false><<<blocks, DVGO_BLOCK, 0, st>>>(P.a, P.b, P.c, C, grad_out, gstride, sum, xyz, xyz_min, xyz_max, M, S.run,
                                                              S.nchunk, S.lanes);
  DVGO_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
