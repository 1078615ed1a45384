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
#include <limits.h>

#include "common.h"

#define TP_RUN_DEFAULT 4

struct TpPlane {
  float* p;
  int H, W;
  int64_t sC, sH, sW;
};
struct TpPlanes { TpPlane a, b, c; };

// plane s of the three and the world axes its rows / columns follow, by selects among three by-value kernel arguments
// (one argument struct holding all three, indexed by s, was copied to scratch: 128 B per lane)
__device__ __forceinline__ TpPlane tp_pick(const TpPlane A, const TpPlane B, const TpPlane D, int s, int& ah, int& aw) {
  ah = (s == 0) ? 1 : (s == 1) ? 0 : 2;
  aw = (s == 0) ? 2 : (s == 1) ? 1 : 0;
  TpPlane q;
  q.p = (s == 0) ? A.p : (s == 1) ? B.p : D.p;
  q.H = (s == 0) ? A.H : (s == 1) ? B.H : D.H;
  q.W = (s == 0) ? A.W : (s == 1) ? B.W : D.W;
  q.sC = (s == 0) ? A.sC : (s == 1) ? B.sC : D.sC;
  q.sH = (s == 0) ? A.sH : (s == 1) ? B.sH : D.sH;
  q.sW = (s == 0) ? A.sW : (s == 1) ? B.sW : D.sW;
  return q;
}

struct BiSetup {
  int h0, w0;            // floor corner (may be -1 or size-1 at the edges)
  float wh0, wh1, ww0, ww1;
};

// floor and weights of one axis: the expressions of dvgo_tri_from_g.  The int conversion is clamped so that a
// coordinate far outside the box cannot overflow h0 + 1; such a corner is out of range either way.
__device__ __forceinline__ void tp_axis(float g, int& i0, float& w0, float& w1) {
  const float f = floorf(g);
  i0 = (int)fminf(fmaxf(f, -1.0e9f), 1.0e9f);
  w0 = (f + 1.0f) - g;
  w1 = g - f;
}

__device__ __forceinline__ BiSetup tp_setup(const float* __restrict__ xyz, const float* __restrict__ mn,
                                            const float* __restrict__ mx, int64_t m, int ah, int aw, int H, int W) {
  BiSetup b;
  tp_axis(dvgo_src_index(xyz[3 * m + ah], mn[ah], mx[ah], H), b.h0, b.wh0, b.wh1);
  tp_axis(dvgo_src_index(xyz[3 * m + aw], mn[aw], mx[aw], W), b.w0, b.ww0, b.ww1);
  return b;
}

template <int VEC> struct TpVal { float v[VEC]; };

template <int VEC>
__device__ __forceinline__ TpVal<VEC> tp_load(const float* __restrict__ p, int64_t sC) {
  TpVal<VEC> r;
  if constexpr (VEC == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w;
  } else {
#pragma unroll
    for (int i = 0; i < VEC; ++i) r.v[i] = p[i * sC];
  }
  return r;
}

// VEC channels from c on of plane q at sample m
template <int VEC>
__device__ __forceinline__ TpVal<VEC> tp_sample(const TpPlane& q, int ah, int aw, int c, const float* __restrict__ xyz,
                                                const float* __restrict__ mn, const float* __restrict__ mx, int64_t m) {
  const BiSetup b = tp_setup(xyz, mn, mx, m, ah, aw, q.H, q.W);
  const int h1 = b.h0 + 1, w1 = b.w0 + 1;
  const bool okh0 = (b.h0 >= 0) & (b.h0 < q.H), okh1 = (h1 >= 0) & (h1 < q.H);
  const bool okw0 = (b.w0 >= 0) & (b.w0 < q.W), okw1 = (w1 >= 0) & (w1 < q.W);
  const int64_t oh0 = (int64_t)min(max(b.h0, 0), q.H - 1) * q.sH, oh1 = (int64_t)min(max(h1, 0), q.H - 1) * q.sH;
  const int64_t ow0 = (int64_t)min(max(b.w0, 0), q.W - 1) * q.sW, ow1 = (int64_t)min(max(w1, 0), q.W - 1) * q.sW;
  const float* base = q.p + (int64_t)c * q.sC;
  const TpVal<VEC> v00 = tp_load<VEC>(base + oh0 + ow0, q.sC), v01 = tp_load<VEC>(base + oh0 + ow1, q.sC);
  const TpVal<VEC> v10 = tp_load<VEC>(base + oh1 + ow0, q.sC), v11 = tp_load<VEC>(base + oh1 + ow1, q.sC);
  const float k00 = b.wh0 * b.ww0, k01 = b.wh0 * b.ww1, k10 = b.wh1 * b.ww0, k11 = b.wh1 * b.ww1;
  TpVal<VEC> r;
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    float acc = 0.f;
    acc = (okh0 & okw0) ? fmaf(v00.v[i], k00, acc) : acc;
    acc = (okh0 & okw1) ? fmaf(v01.v[i], k01, acc) : acc;
    acc = (okh1 & okw0) ? fmaf(v10.v[i], k10, acc) : acc;
    acc = (okh1 & okw1) ? fmaf(v11.v[i], k11, acc) : acc;
    r.v[i] = acc;
  }
  return r;
}

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
  float* o = out + (int64_t)tid * VEC;
  if constexpr (VEC == 4) {
    *reinterpret_cast<float4*>(o) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
  } else {
#pragma unroll
    for (int i = 0; i < VEC; ++i) o[i] = r.v[i];
  }
}

// the four corner sums of cell (h0, w0) -> the plane, out-of-range corners dropped
__device__ __forceinline__ void tp_flush(const TpPlane& q, float* __restrict__ base, int h0, int w0, float a00, float a01,
                                         float a10, float a11) {
  const int h1 = h0 + 1, w1 = w0 + 1;
  const bool okh0 = (h0 >= 0) & (h0 < q.H), okh1 = (h1 >= 0) & (h1 < q.H);
  const bool okw0 = (w0 >= 0) & (w0 < q.W), okw1 = (w1 >= 0) & (w1 < q.W);
  if (okh0 & okw0) atomicAdd(base + (int64_t)h0 * q.sH + (int64_t)w0 * q.sW, a00);
  if (okh0 & okw1) atomicAdd(base + (int64_t)h0 * q.sH + (int64_t)w1 * q.sW, a01);
  if (okh1 & okw0) atomicAdd(base + (int64_t)h1 * q.sH + (int64_t)w0 * q.sW, a10);
  if (okh1 & okw1) atomicAdd(base + (int64_t)h1 * q.sH + (int64_t)w1 * q.sW, a11);
}

// total = nchunk * 3C lanes, nchunk = ceil(M / run).  CFAST: channel fastest (channels-last planes), else sample fastest.
template <bool CFAST>
__global__ void __launch_bounds__(DVGO_BLOCK)
triplane_bwd_kernel(TpPlane PA, TpPlane PB, TpPlane PC, int C, const float* __restrict__ grad_out, int gstride, int sum,
                    const float* __restrict__ xyz, const float* __restrict__ mn, const float* __restrict__ mx,
                    int64_t M, int run, int64_t nchunk, int64_t total) {
  const int64_t tid = (int64_t)blockIdx.x * DVGO_BLOCK + threadIdx.x;
  if (tid >= total) return;
  int64_t chunk;
  int s, c;
  if (CFAST) {
    chunk = tid / (3 * C);
    const int r = (int)(tid - chunk * (3 * C));
    s = r / C;
    c = r - s * C;
  } else {
    const int sc = (int)(tid / nchunk);
    chunk = tid - (int64_t)sc * nchunk;
    s = sc / C;
    c = sc - s * C;
  }
  int ah, aw;
  const TpPlane q = tp_pick(PA, PB, PC, s, ah, aw);
  float* base = q.p + (int64_t)c * q.sC;
  const float* g = grad_out + (sum ? c : s * C + c);
  const int64_t m0 = chunk * run;
  const int64_t m1 = (m0 + run < M) ? m0 + run : M;
  int ch = INT_MIN, cw = INT_MIN;
  float a00 = 0.f, a01 = 0.f, a10 = 0.f, a11 = 0.f;
  for (int64_t m = m0; m < m1; ++m) {
    const BiSetup b = tp_setup(xyz, mn, mx, m, ah, aw, q.H, q.W);
    const float gv = g[m * gstride];
    if ((b.h0 != ch) | (b.w0 != cw)) {
      if (ch != INT_MIN) tp_flush(q, base, ch, cw, a00, a01, a10, a11);
      ch = b.h0; cw = b.w0;
      a00 = a01 = a10 = a11 = 0.f;
    }
    a00 += (b.wh0 * b.ww0) * gv;
    a01 += (b.wh0 * b.ww1) * gv;
    a10 += (b.wh1 * b.ww0) * gv;
    a11 += (b.wh1 * b.ww1) * gv;
  }
  if (ch != INT_MIN) tp_flush(q, base, ch, cw, a00, a01, a10, a11);
}

static bool tp_plane_ok(const TpPlane& q) { return q.H >= 1 && q.W >= 1; }
static bool tp_plane_vec(const TpPlane& q) {
  return q.sC == 1 && (q.sH % 4 == 0 || q.H == 1) && (q.sW % 4 == 0 || q.W == 1) && ((((uintptr_t)q.p) & 15) == 0);
}

static int tp_check(const TpPlanes& P, int C, const void* xyz, const void* mn, const void* mx, int64_t M,
                    const void* io) {
  if (M < 0 || C < 0 || !tp_plane_ok(P.a) || !tp_plane_ok(P.b) || !tp_plane_ok(P.c)) return DVGO_EINVAL;
  if (M == 0 || C == 0) return 1;   // nothing to do
  if (!P.a.p || !P.b.p || !P.c.p || !xyz || !mn || !mx || !io) return DVGO_EINVAL;
  if (!dvgo_fits(M * 3 * (int64_t)C)) return DVGO_ERANGE;
  return 0;
}

#define TP_PLANES(px, py, pz)                                                                   \
  TpPlanes P;                                                                                   \
  P.a = TpPlane{const_cast<float*>(px), H_xy, W_xy, sC_xy, sH_xy, sW_xy};                       \
  P.b = TpPlane{const_cast<float*>(py), H_yz, W_yz, sC_yz, sH_yz, sW_yz};                       \
  P.c = TpPlane{const_cast<float*>(pz), H_zx, W_zx, sC_zx, sH_zx, sW_zx}

extern "C" {

int dvgo_triplane_fwd(const float* xy, int H_xy, int W_xy, int64_t sC_xy, int64_t sH_xy, int64_t sW_xy,
                      const float* yz, int H_yz, int W_yz, int64_t sC_yz, int64_t sH_yz, int64_t sW_yz,
                      const float* zx, int H_zx, int W_zx, int64_t sC_zx, int64_t sH_zx, int64_t sW_zx,
                      int C, const float* xyz, const float* xyz_min, const float* xyz_max, int64_t M, int sum,
                      float* out, void* stream) {
  TP_PLANES(xy, yz, zx);
  const int rc = tp_check(P, C, xyz, xyz_min, xyz_max, M, out);
  if (rc < 0) return rc;
  if (rc == 1) return 0;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (C % 4 == 0) && tp_plane_vec(P.a) && tp_plane_vec(P.b) && tp_plane_vec(P.c) &&
                   ((((uintptr_t)out) & 15) == 0);
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
  TP_PLANES(g_xy, g_yz, g_zx);
  if (run < 0) return DVGO_EINVAL;
  const int rc = tp_check(P, C, xyz, xyz_min, xyz_max, M, grad_out);
  if (rc < 0) return rc;
  if (rc == 1) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (run == 0) run = TP_RUN_DEFAULT;
  const int64_t nchunk = (M + run - 1) / run;
  const int64_t total = nchunk * 3 * C;
  const int blocks = dvgo_blocks(total, DVGO_BLOCK);
  const int gstride = sum ? C : 3 * C;
  if (P.a.sC == 1 && P.b.sC == 1 && P.c.sC == 1 && C > 1)
    triplane_bwd_kernel<true><<<blocks, DVGO_BLOCK, 0, st>>>(P.a, P.b, P.c, C, grad_out, gstride, sum, xyz, xyz_min, xyz_max, M, run,
                                                             nchunk, total);
  else
    triplane_bwd_kernel<false><<<blocks, DVGO_BLOCK, 0, st>>>(P.a, P.b, P.c, C, grad_out, gstride, sum, xyz, xyz_min, xyz_max, M, run,
                                                              nchunk, total);
  DVGO_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
