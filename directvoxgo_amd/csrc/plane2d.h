// What the samplers over three 2-D feature planes share (triplane.hip, plane_rows.hip, liif.hip, vm.hip, vm_density.hip,
// march_vm.hip).
// Device: the plane descriptor, the per-axis floor and weights, the four-corner fma chain, the four-corner atomic flush
// and the run-merging walk of the gradient scatter (include/dvgo_hip.h, the tri-plane block, states the arithmetic).
// Host, below: the pack of the 18 plane scalars of an entry point, the vector-load predicate, the staged argument check,
// the launch shape of a scatter and the coordinate-table numbers of the two decoders.
#pragma once
#include <limits.h>

#include <initializer_list>

#include "common.h"

// samples a lane of a scatter merges before its atomics (run == 0 at the entry points)
#define TP_RUN_DEFAULT 4

struct TpPlane {
  float* p;
  int H, W;
  int64_t sC, sH, sW;
};

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

// the same from values: the sample's coordinates along the rows' and the columns' world axis and the box on those two axes
// (march_vm.hip forms its positions in registers and gets the box as kernel arguments)
__device__ __forceinline__ BiSetup tp_setup(float ph, float pw, float mnh, float mxh, float mnw, float mxw, int H, int W) {
  BiSetup b;
  tp_axis(dvgo_src_index(ph, mnh, mxh, H), b.h0, b.wh0, b.wh1);
  tp_axis(dvgo_src_index(pw, mnw, mxw, W), b.w0, b.ww0, b.ww1);
  return b;
}

template <int VEC> struct TpVal { float v[VEC]; };

template <int VEC>
__device__ __forceinline__ TpVal<VEC> tp_load(const float* __restrict__ p, int64_t sC) {
  TpVal<VEC> r;
  if constexpr (VEC == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w;
  } else if constexpr (VEC == 2) {
    const float2 q = *reinterpret_cast<const float2*>(p);
    r.v[0] = q.x; r.v[1] = q.y;
  } else {
#pragma unroll
    for (int i = 0; i < VEC; ++i) r.v[i] = p[i * sC];
  }
  return r;
}

template <int VEC>
__device__ __forceinline__ void tp_store(float* __restrict__ p, const TpVal<VEC>& r) {
  if constexpr (VEC == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
  } else if constexpr (VEC == 2) {
    *reinterpret_cast<float2*>(p) = make_float2(r.v[0], r.v[1]);
  } else {
#pragma unroll
    for (int i = 0; i < VEC; ++i) p[i] = r.v[i];
  }
}

// tp_sample in two steps, for a caller that needs the corner values as well as the plane value (vm_xyz.hip): the same
// loads, in-range tests and fma chain as tp_sample below, hence the same bits.  (tp_sample is not written in terms of these:
// DESIGN.md section 6o.)
// VEC channels from c on of the four corners of cell (b.h0, b.w0) of plane q, and which corners are in range: the loads
// come from clamped, always valid addresses, and a corner out of range is dropped by whoever blends (zero padding)
template <int VEC>
struct TpCorners {
  bool okh0, okh1, okw0, okw1;
  TpVal<VEC> v00, v01, v10, v11;
};

template <int VEC>
__device__ __forceinline__ TpCorners<VEC> tp_gather(const TpPlane& q, const BiSetup& b, int c) {
  TpCorners<VEC> k;
  const int h1 = b.h0 + 1, w1 = b.w0 + 1;
  k.okh0 = (b.h0 >= 0) & (b.h0 < q.H); k.okh1 = (h1 >= 0) & (h1 < q.H);
  k.okw0 = (b.w0 >= 0) & (b.w0 < q.W); k.okw1 = (w1 >= 0) & (w1 < q.W);
  const int64_t oh0 = (int64_t)min(max(b.h0, 0), q.H - 1) * q.sH, oh1 = (int64_t)min(max(h1, 0), q.H - 1) * q.sH;
  const int64_t ow0 = (int64_t)min(max(b.w0, 0), q.W - 1) * q.sW, ow1 = (int64_t)min(max(w1, 0), q.W - 1) * q.sW;
  const float* base = q.p + (int64_t)c * q.sC;
  k.v00 = tp_load<VEC>(base + oh0 + ow0, q.sC); k.v01 = tp_load<VEC>(base + oh0 + ow1, q.sC);
  k.v10 = tp_load<VEC>(base + oh1 + ow0, q.sC); k.v11 = tp_load<VEC>(base + oh1 + ow1, q.sC);
  return k;
}

// the plane value of channel i of the gathered corners: the fma chain over 00, 01, 10, 11 from 0, corners out of range skipped
template <int VEC>
__device__ __forceinline__ float tp_blend(const TpCorners<VEC>& k, int i, float k00, float k01, float k10, float k11) {
  float acc = 0.f;
  acc = (k.okh0 & k.okw0) ? fmaf(k.v00.v[i], k00, acc) : acc;
  acc = (k.okh0 & k.okw1) ? fmaf(k.v01.v[i], k01, acc) : acc;
  acc = (k.okh1 & k.okw0) ? fmaf(k.v10.v[i], k10, acc) : acc;
  acc = (k.okh1 & k.okw1) ? fmaf(k.v11.v[i], k11, acc) : acc;
  return acc;
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

// the same from values (tp_setup's second form): the same loads, weights and fma chain, hence the same bits
template <int VEC>
__device__ __forceinline__ TpVal<VEC> tp_sample(const TpPlane& q, int c, float ph, float pw, float mnh, float mxh, float mnw,
                                                float mxw) {
  const BiSetup b = tp_setup(ph, pw, mnh, mxh, mnw, mxw, q.H, q.W);
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

// One lane of the gradient scatter of both translation units: lane tid of total = nchunk * 3C owns (a run of `run`
// consecutive samples, plane s, channel c) and reads g[s * plane_off + m * gstride + c]; it keeps the four corner sums of
// the texel cell it is in in registers and flushes them when the cell changes and at the end of its run.
// CFAST: channel fastest (channels-last planes), else sample fastest.
template <bool CFAST>
__device__ __forceinline__ void tp_scatter_lane(const TpPlane PA, const TpPlane PB, const TpPlane PC, int C,
                                                const float* __restrict__ grad, int64_t gstride, int64_t plane_off,
                                                const float* __restrict__ xyz, const float* __restrict__ mn,
                                                const float* __restrict__ mx, int64_t M, int run, int64_t nchunk,
                                                int64_t total) {
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
  const float* g = grad + (int64_t)s * plane_off + c;
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

// ---------------------------------------------------------------------------------------------- host side
struct TpPlanes { TpPlane a, b, c; };

// the three planes of an entry point from its 18 plane scalars, which every entry point names alike
#define TP_PLANES(px, py, pz)                                                           \
  TpPlanes{TpPlane{const_cast<float*>(px), H_xy, W_xy, sC_xy, sH_xy, sW_xy},            \
           TpPlane{const_cast<float*>(py), H_yz, W_yz, sC_yz, sH_yz, sW_yz},            \
           TpPlane{const_cast<float*>(pz), H_zx, W_zx, sC_zx, sH_zx, sW_zx}}

static bool tp_plane_ok(const TpPlane& q) { return q.H >= 1 && q.W >= 1; }

// a texel's channels can be read V floats at a time: channels-last, every texel and the base on a 4 V byte boundary
static bool tp_plane_vec(const TpPlane& q, int V) {
  return q.sC == 1 && (q.sH % V == 0 || q.H == 1) && (q.sW % V == 0 || q.W == 1) && ((((uintptr_t)q.p) & (4 * V - 1)) == 0);
}
static bool tp_planes_vec(const TpPlanes& P, int V) { return tp_plane_vec(P.a, V) && tp_plane_vec(P.b, V) && tp_plane_vec(P.c, V); }

// The argument check of every entry point that takes three planes.  < 0: the error; 1: nothing to do; 0: launch.
// The stages and their order are the contract (tests/test_plane_entries_host.py): shapes, among them the caller's own
// (`shape`: world extents, P, line lengths); M == 0 or C == 0, with no pointer looked at; NULL pointers, among them the
// caller's own (`ptrs`); the 32-bit range of what a launch indexes, a sample's `rows` rows of `row` floats.
static int tp_check(const TpPlanes& P, int C, int64_t M, bool shape, const void* xyz, const void* mn, const void* mx,
                    std::initializer_list<const void*> ptrs, int rows, int64_t row) {
  if (M < 0 || C < 0 || !tp_plane_ok(P.a) || !tp_plane_ok(P.b) || !tp_plane_ok(P.c) || !shape) return DVGO_EINVAL;
  if (M == 0 || C == 0) return 1;
  bool null = !P.a.p || !P.b.p || !P.c.p || !xyz || !mn || !mx;
  for (const void* p : ptrs) null = null || !p;
  if (null) return DVGO_EINVAL;
  if (!dvgo_fits(row) || !dvgo_fits(M * rows * row)) return DVGO_ERANGE;
  return 0;
}

// The launch shape of a gradient scatter: a lane merges `run` consecutive samples (0: `run_default`), nchunk = ceil(M / run)
// runs times `per` lanes each; channel fastest when every plane is channels-last, else sample fastest.
struct TpScatter {
  int run;
  int64_t nchunk, lanes;
  bool cfast;
};

static TpScatter tp_scatter(const TpPlanes& P, int C, int64_t M, int run, int run_default, int per) {
  TpScatter s;
  s.run = run ? run : run_default;
  s.nchunk = (M + s.run - 1) / s.run;
  s.lanes = s.nchunk * per;
  s.cfast = P.a.sC == 1 && P.b.sC == 1 && P.c.sC == 1 && C > 1;
  return s;
}

// the coordinate table a plane is decoded against: Ta rows, Tb columns (two world_size extents)
struct PrTable {
  int Ta, Tb;
  float sa, sb;          // 2 / (Ta - 1), 2 / (Tb - 1)   (0 when the extent is 1: node = -1)
  float ra, rb;          // 1 / Ta, 1 / Tb
};

static PrTable pr_table(int Ta, int Tb) {
  PrTable t;
  t.Ta = Ta; t.Tb = Tb;
  t.sa = (Ta > 1) ? 2.0f / (float)(Ta - 1) : 0.0f;
  t.sb = (Tb > 1) ? 2.0f / (float)(Tb - 1) : 0.0f;
  t.ra = 1.0f / (float)Ta; t.rb = 1.0f / (float)Tb;
  return t;
}
