// Bilinear plane decoder, everything in front of its MLPs: lib/tri_dvgo.py:568-607 interpolate (implicit_voxel_feat=True,
// liif=False) without the Interp_MLP calls.  Per call the reference runs three F.grid_sample on the planes, rebuilds three
// two-channel coordinate tables (make_coord) and runs three more F.grid_sample on them, encodes the sampled coordinates
// (sin / cos of q * 2^j) and concatenates the MLP input row.  Here: one kernel writes the rows, one scatters the gradient
// of their feature columns into the planes.  include/dvgo_hip.h states the arithmetic.
//
// Rows: bound by the `inp` write (3 D floats per sample against 12 B of position read and planes that stay in L2).  A
// launch covers one plane's slab [M, D] per blockIdx.y; a lane owns VEC consecutive floats of one row, so a wave's stores
// are 64 consecutive pieces of `inp`.  C % VEC == 0, so a piece is either VEC channels of the bilinear sample (plane2d.h:
// triplane.hip's corner walk, four 16- or 8-byte loads when the planes are channels-last) or part of the row's tail
// (q0, q1, the 2P sines, the 2P cosines[, cell_a, cell_b]).  The coordinate table is never built: its value at a corner
// is node_T of the corner's index.  Every lane recomputes the sample's geometry.
//
// Scatter: the walk triplane.hip uses (plane2d.h: tp_scatter_lane), reading its gradient from the first C columns of the
// rows: 12 C float atomics per sample at most, a lane owns (a run of consecutive samples, plane, channel) and keeps the
// four corner sums of its texel cell in registers.  Lane order and run default as there.
#include "common.h"
#include "plane2d.h"

__device__ __forceinline__ PrTable pr_pick(const PrTable A, const PrTable B, const PrTable D, int s) {
  PrTable t;
  t.Ta = (s == 0) ? A.Ta : (s == 1) ? B.Ta : D.Ta;
  t.Tb = (s == 0) ? A.Tb : (s == 1) ? B.Tb : D.Tb;
  t.sa = (s == 0) ? A.sa : (s == 1) ? B.sa : D.sa;
  t.sb = (s == 0) ? A.sb : (s == 1) ? B.sb : D.sb;
  t.ra = (s == 0) ? A.ra : (s == 1) ? B.ra : D.ra;
  t.rb = (s == 0) ? A.rb : (s == 1) ? B.rb : D.rb;
  return t;
}

__device__ __forceinline__ float pr_node(int i, float step) { return (float)i * step - 1.0f; }

// (q0, q1): the bilinear sample of the table at the sample, plane2d.h's corner order and fma chain from 0; channel 0
// holds the column's node, channel 1 the row's
__device__ __forceinline__ void pr_coord(const PrTable& t, int ah, int aw, const float* __restrict__ xyz,
                                         const float* __restrict__ mn, const float* __restrict__ mx, int64_t m, float& q0,
                                         float& q1) {
  const BiSetup b = tp_setup(xyz, mn, mx, m, ah, aw, t.Ta, t.Tb);
  const int h1 = b.h0 + 1, w1 = b.w0 + 1;
  const bool okh0 = (b.h0 >= 0) & (b.h0 < t.Ta), okh1 = (h1 >= 0) & (h1 < t.Ta);
  const bool okw0 = (b.w0 >= 0) & (b.w0 < t.Tb), okw1 = (w1 >= 0) & (w1 < t.Tb);
  const float nh0 = pr_node(b.h0, t.sa), nh1 = pr_node(h1, t.sa);
  const float nw0 = pr_node(b.w0, t.sb), nw1 = pr_node(w1, t.sb);
  const float k00 = b.wh0 * b.ww0, k01 = b.wh0 * b.ww1, k10 = b.wh1 * b.ww0, k11 = b.wh1 * b.ww1;
  float a = 0.f, r = 0.f;
  a = (okh0 & okw0) ? fmaf(nw0, k00, a) : a;   r = (okh0 & okw0) ? fmaf(nh0, k00, r) : r;
  a = (okh0 & okw1) ? fmaf(nw1, k01, a) : a;   r = (okh0 & okw1) ? fmaf(nh0, k01, r) : r;
  a = (okh1 & okw0) ? fmaf(nw0, k10, a) : a;   r = (okh1 & okw0) ? fmaf(nh1, k10, r) : r;
  a = (okh1 & okw1) ? fmaf(nw1, k11, a) : a;   r = (okh1 & okw1) ? fmaf(nh1, k11, r) : r;
  q0 = a;
  q1 = r;
}

// element k of a row's tail: q0, q1, sinf(q_i * 2^j) for (i, j) i-major, cosf of the same, cell_a, cell_b
__device__ __forceinline__ float pr_tail(int k, int P, float q0, float q1, const PrTable& t) {
  if (k < 2) return k == 0 ? q0 : q1;
  k -= 2;
  if (k >= 4 * P) return k == 4 * P ? t.ra : t.rb;
  const bool cosine = k >= 2 * P;
  k -= cosine ? 2 * P : 0;
  const bool second = k >= P;
  const int j = k - (second ? P : 0);
  const float arg = ldexpf(second ? q1 : q0, j);         // q * 2^j, exact
  return cosine ? cosf(arg) : sinf(arg);
}

// blockIdx.y = s; per = M * (D / VEC) lanes in x (< 2^31: the entry checks 3 M D)
template <int VEC>
__global__ void __launch_bounds__(DVGO_BLOCK)
plane_rows_fwd_kernel(TpPlane PA, TpPlane PB, TpPlane PC, PrTable TA, PrTable TB, PrTable TC, int C, int D, int P,
                      const float* __restrict__ xyz, const float* __restrict__ mn, const float* __restrict__ mx,
                      unsigned int M, unsigned int per, float* __restrict__ inp) {
  const unsigned int tid = blockIdx.x * (unsigned int)DVGO_BLOCK + threadIdx.x;
  if (tid >= per) return;
  const int s = (int)blockIdx.y;
  const unsigned int G = (unsigned int)D / VEC;
  const unsigned int m = tid / G;
  const int c = (int)(tid - m * G) * VEC;
  int ah, aw;
  const TpPlane q = tp_pick(PA, PB, PC, s, ah, aw);
  float* o = inp + ((int64_t)s * M + m) * D + c;
  TpVal<VEC> r;
  if (c < C) {
    r = tp_sample<VEC>(q, ah, aw, c, xyz, mn, mx, m);
  } else {
    const PrTable t = pr_pick(TA, TB, TC, s);
    float q0, q1;
    pr_coord(t, ah, aw, xyz, mn, mx, m, q0, q1);
#pragma unroll
    for (int i = 0; i < VEC; ++i) r.v[i] = pr_tail(c - C + i, P, q0, q1, t);
  }
  tp_store<VEC>(o, r);
}

// total = nchunk * 3C lanes, nchunk = ceil(M / run): plane2d.h's walk over rows of D floats, plane s's slab M * D floats
// behind the one before; c < C, so the columns behind the features are never read
template <bool CFAST>
__global__ void __launch_bounds__(DVGO_BLOCK)
plane_rows_bwd_kernel(TpPlane PA, TpPlane PB, TpPlane PC, int C, int D, const float* __restrict__ ginp,
                      const float* __restrict__ xyz, const float* __restrict__ mn, const float* __restrict__ mx,
                      int64_t M, int run, int64_t nchunk, int64_t total) {
  tp_scatter_lane<CFAST>(PA, PB, PC, C, ginp, D, M * D, xyz, mn, mx, M, run, nchunk, total);
}

// a row's floats
static int64_t pr_width(int C, int P, int cell_decode) { return (int64_t)C + 2 + 4 * (int64_t)P + (cell_decode ? 2 : 0); }

// tp_check with this decoder's shapes: the world extents and P
static int pr_check(const TpPlanes& Q, int C, int64_t M, int Wx, int Wy, int Wz, int P, const void* xyz, const void* mn,
                    const void* mx, const void* io, int64_t D) {
  return tp_check(Q, C, M, Wx >= 1 && Wy >= 1 && Wz >= 1 && P >= 1, xyz, mn, mx, {io}, 3, D);
}

extern "C" {

int dvgo_plane_rows_fwd(const float* xy, int H_xy, int W_xy, int64_t sC_xy, int64_t sH_xy, int64_t sW_xy,
                        const float* yz, int H_yz, int W_yz, int64_t sC_yz, int64_t sH_yz, int64_t sW_yz,
                        const float* zx, int H_zx, int W_zx, int64_t sC_zx, int64_t sH_zx, int64_t sW_zx,
                        int C, const float* xyz, const float* xyz_min, const float* xyz_max, int64_t M,
                        int Wx, int Wy, int Wz, int P, int cell_decode, float* inp, void* stream) {
  const TpPlanes Q = TP_PLANES(xy, yz, zx);
  const int64_t D = pr_width(C, P, cell_decode);
  const int rc = pr_check(Q, C, M, Wx, Wy, Wz, P, xyz, xyz_min, xyz_max, inp, D);
  if (rc) return rc < 0 ? rc : 0;
  hipStream_t st = (hipStream_t)stream;
  const PrTable TA = pr_table(Wx, Wy), TB = pr_table(Wy, Wz), TC = pr_table(Wz, Wx);
  int vec = 1;
  if (C % 4 == 0 && D % 4 == 0 && tp_planes_vec(Q, 4) && ((((uintptr_t)inp) & 15) == 0))
    vec = 4;
  else if (C % 2 == 0 && D % 2 == 0 && tp_planes_vec(Q, 2) && ((((uintptr_t)inp) & 7) == 0))
    vec = 2;
  const unsigned int per = (unsigned int)(M * (D / vec));
  const dim3 grid((unsigned int)dvgo_blocks(per, DVGO_BLOCK), 3u);
  if (vec == 4)
    plane_rows_fwd_kernel<4><<<grid, DVGO_BLOCK, 0, st>>>(Q.a, Q.b, Q.c, TA, TB, TC, C, (int)D, P, xyz, xyz_min, xyz_max, (unsigned int)M, per, inp);
  else if (vec == 2)
    plane_rows_fwd_kernel<2><<<grid, DVGO_BLOCK, 0, st>>>(Q.a, Q.b, Q.c, TA, TB, TC, C, (int)D, P, xyz, xyz_min, xyz_max, (unsigned int)M, per, inp);
  else
    plane_rows_fwd_kernel<1><<<grid, DVGO_BLOCK, 0, st>>>(Q.a, Q.b, Q.c, TA, TB, TC, C, (int)D, P, xyz, xyz_min, xyz_max, (unsigned int)M, per, inp);
  DVGO_LAUNCH_CHECK();
  return 0;
}

int dvgo_plane_rows_bwd(const float* grad_inp,
                        float* g_xy, int H_xy, int W_xy, int64_t sC_xy, int64_t sH_xy, int64_t sW_xy,
                        float* g_yz, int H_yz, int W_yz, int64_t sC_yz, int64_t sH_yz, int64_t sW_yz,
                        float* g_zx, int H_zx, int W_zx, int64_t sC_zx, int64_t sH_zx, int64_t sW_zx,
                        int C, const float* xyz, const float* xyz_min, const float* xyz_max, int64_t M,
                        int Wx, int Wy, int Wz, int P, int cell_decode, int run, void* stream) {
  const TpPlanes Q = TP_PLANES(g_xy, g_yz, g_zx);
  const int64_t D = pr_width(C, P, cell_decode);
  if (run < 0) return DVGO_EINVAL;
  const int rc = pr_check(Q, C, M, Wx, Wy, Wz, P, xyz, xyz_min, xyz_max, grad_inp, D);
  if (rc) return rc < 0 ? rc : 0;
  hipStream_t st = (hipStream_t)stream;
  const TpScatter S = tp_scatter(Q, C, M, run, TP_RUN_DEFAULT, 3 * C);
  const int blocks = dvgo_blocks(S.lanes, DVGO_BLOCK);
  if (S.cfast)
    plane_rows_bwd_kernel<true><<<blocks, DVGO_BLOCK, 0, st>>>(Q.a, Q.b, Q.c, C, (int)D, grad_inp, xyz, xyz_min, xyz_max, M, S.run, S.nchunk, S.lanes);
  else
    plane_rows_bwd_kernel<false><<<blocks, DVGO_BLOCK, 0, st>>>(Q.a, Q.b, Q.c, C, (int)D, grad_inp, xyz, xyz_min, xyz_max, M, S.run, S.nchunk, S.lanes);
  DVGO_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
