// LIIF plane decoder, everything around its GEMMs: lib/tri_dvgo.py:481-565 liif_interpolate without the Interp_MLP calls.
// For each sample, plane and shifted position (E = 4 with local_ensemble, else 1) the reference clones the coordinates,
// shifts and clamps them, runs two F.grid_sample(mode='nearest', align_corners=False) (features, coordinate table),
// permutes, concatenates the MLP input row, and afterwards stacks and blends the E predictions by the opposite corner's
// area.  Here: one gather kernel writes the rows and the blend weights, one blend kernel sums the predictions, and each
// has its gradient (the scatter into the nearest texels; grad_pred = g * wgt).  include/dvgo_hip.h states the arithmetic.
//
// Gather: bound by the `inp` write (3 E D floats per sample against 12 B of position read and planes that stay in L2).
// A launch covers one (plane, shift) slab [M, D] per blockIdx.y; a lane owns VEC consecutive floats of one row, so a
// wave's stores are 64 consecutive pieces of `inp`.  C % VEC == 0, so a piece is either VEC channels of the nearest texel
// (one 16- or 8-byte load when the planes are channels-last) or part of the row's tail (rel0, rel1[, cell0, cell1]).
// Every lane recomputes the sample's geometry (two divisions, a dozen multiply-adds); the lane that stores rel0 also
// evaluates the other shifts' areas and stores the sample's blend weight.
//
// Scatter: E * 3 C float atomics per sample at most.  A lane owns (a run of consecutive samples, plane, shift, channel)
// and sums in a register while the nearest texel stays the same: consecutive kept samples of a ray are half a voxel
// apart.  Lane order as in triplane_bwd_kernel: channel fastest when every plane is channels-last, else sample fastest.
#include "common.h"
#include "plane2d.h"

// samples a lane of the scatter merges before its atomics.  Started as a guess (triplane.hip's value); measured at M = 131 072
// it takes 0.35-0.57 of the unmerged time and 8 is 10-14 % faster still (profiles/liif/README.md): short batches not measured yet
#define LF_RUN_DEFAULT 4

struct LfPlane {
  float* p;
  int H, W;
  int64_t sC, sH, sW;
  int Ta, Tb;            // sizes of the coordinate table the plane is decoded against (two world_size extents)
  float ra, rb;          // 1 / Ta, 1 / Tb
  float sa, sb;          // 2 / (Ta - 1), 2 / (Tb - 1)   (0 when the extent is 1: node = -1)
};

// plane s and the world axes its u (rows) and v (columns) follow; s is uniform over a block: scalar selects
__device__ __forceinline__ LfPlane lf_pick(const LfPlane A, const LfPlane B, const LfPlane D, int s, int& au, int& av) {
  au = (s == 0) ? 2 : (s == 1) ? 1 : 0;
  av = (s == 0) ? 1 : (s == 1) ? 0 : 2;
  LfPlane q;
  q.p = (s == 0) ? A.p : (s == 1) ? B.p : D.p;
  q.H = (s == 0) ? A.H : (s == 1) ? B.H : D.H;
  q.W = (s == 0) ? A.W : (s == 1) ? B.W : D.W;
  q.sC = (s == 0) ? A.sC : (s == 1) ? B.sC : D.sC;
  q.sH = (s == 0) ? A.sH : (s == 1) ? B.sH : D.sH;
  q.sW = (s == 0) ? A.sW : (s == 1) ? B.sW : D.sW;
  q.Ta = (s == 0) ? A.Ta : (s == 1) ? B.Ta : D.Ta;
  q.Tb = (s == 0) ? A.Tb : (s == 1) ? B.Tb : D.Tb;
  q.ra = (s == 0) ? A.ra : (s == 1) ? B.ra : D.ra;
  q.rb = (s == 0) ? A.rb : (s == 1) ? B.rb : D.rb;
  q.sa = (s == 0) ? A.sa : (s == 1) ? B.sa : D.sa;
  q.sb = (s == 0) ? A.sb : (s == 1) ? B.sb : D.sb;
  return q;
}

__device__ __forceinline__ float lf_norm(float p, float mn, float mx) { return ((p - mn) / (mx - mn)) * 2.0f - 1.0f; }

// F.grid_sample(mode='nearest', align_corners=False): rint (half to even) of the unnormalised coordinate; clipped, so
// that no coordinate, NaN included, leaves the plane
__device__ __forceinline__ int lf_near(float c, int S) {
  const float r = rintf(((c + 1.0f) * (float)S - 1.0f) / 2.0f);
  return (int)fminf(fmaxf(r, 0.0f), (float)(S - 1));
}

// shift of position e along one axis: +-(1 / T) + 1e-6 with local_ensemble, else 0
__device__ __forceinline__ float lf_shift(bool plus, float r, bool ensemble) {
  return ensemble ? ((plus ? r : -r) + 1e-6f) : 0.0f;
}

__device__ __forceinline__ float lf_clamp(float c) { return fminf(fmaxf(c, (float)(-1 + 1e-6)), (float)(1 - 1e-6)); }

struct LfGeo { int row, col; float rel0, rel1; };

// the clamped shifted position's nearest texel, and the relative coordinates to the table's nearest node
__device__ __forceinline__ LfGeo lf_geo(const LfPlane& q, float u, float v, int e, bool ensemble) {
  const float uc = lf_clamp(u + lf_shift((e & 2) != 0, q.ra, ensemble));
  const float vc = lf_clamp(v + lf_shift((e & 1) != 0, q.rb, ensemble));
  LfGeo g;
  g.row = lf_near(uc, q.H);
  g.col = lf_near(vc, q.W);
  const float q0 = (float)lf_near(vc, q.Tb) * q.sb - 1.0f;
  const float q1 = (float)lf_near(uc, q.Ta) * q.sa - 1.0f;
  g.rel0 = (u - q0) * (float)q.H;
  g.rel1 = (v - q1) * (float)q.W;
  return g;
}

__device__ __forceinline__ float lf_area(const LfGeo& g) { return fabsf(g.rel0 * g.rel1) + 1e-9f; }

// wgt of shift e: the area of shift E - 1 - e over the sum of all, summed in shift order
__device__ __forceinline__ float lf_weight(const LfPlane& q, float u, float v, int e, bool ensemble) {
  if (!ensemble) {
    const float a = lf_area(lf_geo(q, u, v, 0, false));
    return a / a;
  }
  const float a0 = lf_area(lf_geo(q, u, v, 0, true)), a1 = lf_area(lf_geo(q, u, v, 1, true));
  const float a2 = lf_area(lf_geo(q, u, v, 2, true)), a3 = lf_area(lf_geo(q, u, v, 3, true));
  const float tot = ((a0 + a1) + a2) + a3;
  const float mine = (e == 0) ? a3 : (e == 1) ? a2 : (e == 2) ? a1 : a0;
  return mine / tot;
}

// blockIdx.y = s * E + e; per = M * (D / VEC) lanes in x (< 2^31: the entry checks 3 E M D)
template <int VEC>
__global__ void __launch_bounds__(DVGO_BLOCK)
liif_gather_kernel(LfPlane PA, LfPlane PB, LfPlane PC, int C, int D, int E, const float* __restrict__ xyz,
                   const float* __restrict__ mn, const float* __restrict__ mx, unsigned int M, unsigned int per,
                   float* __restrict__ inp, float* __restrict__ wgt) {
  const unsigned int tid = blockIdx.x * (unsigned int)DVGO_BLOCK + threadIdx.x;
  if (tid >= per) return;
  const int se = (int)blockIdx.y;
  const int s = se / E, e = se - s * E;
  const bool ensemble = E > 1;
  const unsigned int G = (unsigned int)D / VEC;
  const unsigned int m = tid / G;
  const int c = (int)(tid - m * G) * VEC;
  int au, av;
  const LfPlane q = lf_pick(PA, PB, PC, s, au, av);
  const float u = lf_norm(xyz[3 * (int64_t)m + au], mn[au], mx[au]);
  const float v = lf_norm(xyz[3 * (int64_t)m + av], mn[av], mx[av]);
  const LfGeo g = lf_geo(q, u, v, e, ensemble);
  float* o = inp + ((int64_t)se * M + m) * D + c;
  if (c < C) {
    const float* t = q.p + (int64_t)c * q.sC + (int64_t)g.row * q.sH + (int64_t)g.col * q.sW;
    tp_store<VEC>(o, tp_load<VEC>(t, q.sC));
    return;
  }
  const int k = c - C;                                   // 0 .. D - C - 1, a multiple of VEC
  const float cell0 = q.ra * (float)q.H, cell1 = q.rb * (float)q.W;
  if constexpr (VEC == 4) {
    *reinterpret_cast<float4*>(o) = make_float4(g.rel0, g.rel1, cell0, cell1);
  } else if constexpr (VEC == 2) {
    *reinterpret_cast<float2*>(o) = (k == 0) ? make_float2(g.rel0, g.rel1) : make_float2(cell0, cell1);
  } else {
    o[0] = (k == 0) ? g.rel0 : (k == 1) ? g.rel1 : (k == 2) ? cell0 : cell1;
  }
  if (k == 0) wgt[(int64_t)se * M + m] = lf_weight(q, u, v, e, ensemble);
}

// blockIdx.y = s * E + e; per = nchunk * C lanes in x, nchunk = ceil(M / run).  CFAST: channel fastest.
template <bool CFAST>
__global__ void __launch_bounds__(DVGO_BLOCK)
liif_scatter_kernel(LfPlane PA, LfPlane PB, LfPlane PC, int C, int D, int E, const float* __restrict__ ginp,
                    const float* __restrict__ xyz, const float* __restrict__ mn, const float* __restrict__ mx, int64_t M,
                    int run, int64_t nchunk, int64_t per) {
  const int64_t tid = (int64_t)blockIdx.x * DVGO_BLOCK + threadIdx.x;
  if (tid >= per) return;
  const int se = (int)blockIdx.y;
  const int s = se / E, e = se - s * E;
  const bool ensemble = E > 1;
  int64_t chunk;
  int c;
  if (CFAST) {
    chunk = tid / C;
    c = (int)(tid - chunk * C);
  } else {
    c = (int)(tid / nchunk);
    chunk = tid - (int64_t)c * nchunk;
  }
  int au, av;
  const LfPlane q = lf_pick(PA, PB, PC, s, au, av);
  float* base = q.p + (int64_t)c * q.sC;
  const float* g = ginp + (int64_t)se * M * D + c;
  const float mnu = mn[au], mxu = mx[au], mnv = mn[av], mxv = mx[av];
  const int64_t m0 = chunk * run;
  const int64_t m1 = (m0 + run < M) ? m0 + run : M;
  int cr = -1, cc = -1;
  float acc = 0.f;
  for (int64_t m = m0; m < m1; ++m) {
    const float u = lf_norm(xyz[3 * m + au], mnu, mxu), v = lf_norm(xyz[3 * m + av], mnv, mxv);
    const LfGeo t = lf_geo(q, u, v, e, ensemble);
    const float gv = g[m * D];
    if ((t.row != cr) | (t.col != cc)) {
      if (cr >= 0) atomicAdd(base + (int64_t)cr * q.sH + (int64_t)cc * q.sW, acc);
      cr = t.row; cc = t.col;
      acc = 0.f;
    }
    acc += gv;
  }
  if (cr >= 0) atomicAdd(base + (int64_t)cr * q.sH + (int64_t)cc * q.sW, acc);
}

// sum over the shifts of plane s at sample m, channels c .. c + VEC: acc = fmaf(pred, wgt, acc) from 0, in shift order
template <int VEC>
__device__ __forceinline__ TpVal<VEC> lf_blend(const float* __restrict__ pred, const float* __restrict__ wgt, int C,
                                               int64_t M, int E, int s, int64_t m, int c) {
  TpVal<VEC> acc;
#pragma unroll
  for (int i = 0; i < VEC; ++i) acc.v[i] = 0.f;
  for (int e = 0; e < E; ++e) {
    const int64_t row = (int64_t)(s * E + e) * M + m;
    const float w = wgt[row];
    const TpVal<VEC> p = tp_load<VEC>(pred + row * C + c, 1);
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc.v[i] = fmaf(p.v[i], w, acc.v[i]);
  }
  return acc;
}

// total = M * (SUM ? C : 3C) / VEC lanes
template <int VEC, bool SUM>
__global__ void __launch_bounds__(DVGO_BLOCK)
liif_blend_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ wgt, int C, int64_t M, int E,
                      unsigned int total, float* __restrict__ out) {
  const unsigned int tid = blockIdx.x * (unsigned int)DVGO_BLOCK + threadIdx.x;
  if (tid >= total) return;
  const unsigned int cg = (unsigned int)C / VEC;
  const unsigned int per = SUM ? cg : 3u * cg;
  const unsigned int m = tid / per, j = tid - m * per;
  TpVal<VEC> r;
  if (SUM) {
    const int c = (int)j * VEC;
    const TpVal<VEC> a = lf_blend<VEC>(pred, wgt, C, M, E, 0, m, c);
    const TpVal<VEC> b = lf_blend<VEC>(pred, wgt, C, M, E, 1, m, c);
    const TpVal<VEC> d = lf_blend<VEC>(pred, wgt, C, M, E, 2, m, c);
#pragma unroll
    for (int i = 0; i < VEC; ++i) r.v[i] = (a.v[i] + b.v[i]) + d.v[i];
  } else {
    const unsigned int s = j / cg;
    r = lf_blend<VEC>(pred, wgt, C, M, E, (int)s, m, (int)(j - s * cg) * VEC);
  }
  tp_store<VEC>(out + (int64_t)tid * VEC, r);
}

// blockIdx.y = s * E + e; per = M * C / VEC lanes in x: grad_pred[s, e, m, c] = grad_out[m, c'] * wgt[s, e, m]
template <int VEC>
__global__ void __launch_bounds__(DVGO_BLOCK)
liif_blend_bwd_kernel(const float* __restrict__ gout, const float* __restrict__ wgt, int C, int64_t M, int E, int sum,
                      unsigned int per, float* __restrict__ gpred) {
  const unsigned int tid = blockIdx.x * (unsigned int)DVGO_BLOCK + threadIdx.x;
  if (tid >= per) return;
  const int se = (int)blockIdx.y;
  const int s = se / E;
  const unsigned int cg = (unsigned int)C / VEC;
  const unsigned int m = tid / cg;
  const int c = (int)(tid - m * cg) * VEC;
  const float w = wgt[(int64_t)se * M + m];
  const TpVal<VEC> g = tp_load<VEC>(gout + (sum ? (int64_t)m * C + c : (int64_t)m * 3 * C + s * C + c), 1);
  TpVal<VEC> r;
#pragma unroll
  for (int i = 0; i < VEC; ++i) r.v[i] = g.v[i] * w;
  tp_store<VEC>(gpred + ((int64_t)se * M + m) * C + c, r);
}

// plane q and the coordinate table it is decoded against (plane2d.h: pr_table)
static LfPlane lf_plane(const TpPlane& q, int Ta, int Tb) {
  const PrTable t = pr_table(Ta, Tb);
  return LfPlane{q.p, q.H, q.W, q.sC, q.sH, q.sW, Ta, Tb, t.ra, t.rb, t.sa, t.sb};
}

// tp_check with this decoder's shapes, the world extents; a sample has 3 E rows of D floats
static int lf_check(const TpPlanes& Q, int C, int64_t M, int Wx, int Wy, int Wz, const void* xyz, const void* mn,
                    const void* mx, std::initializer_list<const void*> io, int D, int E) {
  return tp_check(Q, C, M, Wx >= 1 && Wy >= 1 && Wz >= 1, xyz, mn, mx, io, 3 * E, D);
}

static int lf_blend_check(const void* a, const void* b, const void* c, int C, int64_t M, int E) {
  if (M < 0 || C < 0 || (E != 1 && E != 4)) return DVGO_EINVAL;
  if (M == 0 || C == 0) return 1;
  if (!a || !b || !c) return DVGO_EINVAL;
  if (!dvgo_fits(M * 3 * E * (int64_t)C)) return DVGO_ERANGE;
  return 0;
}

static bool lf_al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

extern "C" {

int dvgo_liif_gather(const float* xy, int H_xy, int W_xy, int64_t sC_xy, int64_t sH_xy, int64_t sW_xy,
                     const float* yz, int H_yz, int W_yz, int64_t sC_yz, int64_t sH_yz, int64_t sW_yz,
                     const float* zx, int H_zx, int W_zx, int64_t sC_zx, int64_t sH_zx, int64_t sW_zx,
                     int C, const float* xyz, const float* xyz_min, const float* xyz_max, int64_t M,
                     int Wx, int Wy, int Wz, int cell_decode, int local_ensemble, float* inp, float* wgt, void* stream) {
  const TpPlanes Q = TP_PLANES(xy, yz, zx);
  const int D = C + (cell_decode ? 4 : 2), E = local_ensemble ? 4 : 1;
  const int rc = lf_check(Q, C, M, Wx, Wy, Wz, xyz, xyz_min, xyz_max, {inp, wgt}, D, E);
  if (rc) return rc < 0 ? rc : 0;
  hipStream_t st = (hipStream_t)stream;
  const LfPlane A = lf_plane(Q.a, Wx, Wy), B = lf_plane(Q.b, Wy, Wz), P = lf_plane(Q.c, Wz, Wx);
  int vec = 1;
  if (C % 4 == 0 && D % 4 == 0 && tp_planes_vec(Q, 4) && lf_al16(inp)) vec = 4;
  else if (C % 2 == 0 && tp_planes_vec(Q, 2) && ((((uintptr_t)inp) & 7) == 0)) vec = 2;
  const unsigned int per = (unsigned int)(M * (D / vec));
  const dim3 grid((unsigned int)dvgo_blocks(per, DVGO_BLOCK), (unsigned int)(3 * E));
  if (vec == 4)
    liif_gather_kernel<4><<<grid, DVGO_BLOCK, 0, st>>>(A, B, P, C, D, E, xyz, xyz_min, xyz_max, (unsigned int)M, per, inp, wgt);
  else if (vec == 2)
    liif_gather_kernel<2><<<grid, DVGO_BLOCK, 0, st>>>(A, B, P, C, D, E, xyz, xyz_min, xyz_max, (unsigned int)M, per, inp, wgt);
  else
    liif_gather_kernel<1><<<grid, DVGO_BLOCK, 0, st>>>(A, B, P, C, D, E, xyz, xyz_min, xyz_max, (unsigned int)M, per, inp, wgt);
  DVGO_LAUNCH_CHECK();
  return 0;
}

int dvgo_liif_scatter(const float* grad_inp,
                      float* g_xy, int H_xy, int W_xy, int64_t sC_xy, int64_t sH_xy, int64_t sW_xy,
                      float* g_yz, int H_yz, int W_yz, int64_t sC_yz, int64_t sH_yz, int64_t sW_yz,
                      float* g_zx, int H_zx, int W_zx, int64_t sC_zx, int64_t sH_zx, int64_t sW_zx,
                      int C, const float* xyz, const float* xyz_min, const float* xyz_max, int64_t M,
                      int Wx, int Wy, int Wz, int cell_decode, int local_ensemble, int run, void* stream) {
  const TpPlanes Q = TP_PLANES(g_xy, g_yz, g_zx);
  const int D = C + (cell_decode ? 4 : 2), E = local_ensemble ? 4 : 1;
  if (run < 0) return DVGO_EINVAL;
  const int rc = lf_check(Q, C, M, Wx, Wy, Wz, xyz, xyz_min, xyz_max, {grad_inp}, D, E);
  if (rc) return rc < 0 ? rc : 0;
  hipStream_t st = (hipStream_t)stream;
  const LfPlane A = lf_plane(Q.a, Wx, Wy), B = lf_plane(Q.b, Wy, Wz), P = lf_plane(Q.c, Wz, Wx);
  const TpScatter S = tp_scatter(Q, C, M, run, LF_RUN_DEFAULT, C);       // one (plane, shift) per blockIdx.y
  const dim3 grid((unsigned int)dvgo_blocks(S.lanes, DVGO_BLOCK), (unsigned int)(3 * E));
  if (S.cfast)
    liif_scatter_kernel<true><<<grid, DVGO_BLOCK, 0, st>>>(A, B, P, C, D, E, grad_inp, xyz, xyz_min, xyz_max, M, S.run, S.nchunk, S.lanes);
  else
    liif_scatter_kernel<false><<<grid, DVGO_BLOCK, 0, st>>>(A, B, P, C, D, E, grad_inp, xyz, xyz_min, xyz_max, M, S.run, S.nchunk, S.lanes);
  DVGO_LAUNCH_CHECK();
  return 0;
}

int dvgo_liif_blend_fwd(const float* pred, const float* wgt, int C, int64_t M, int E, int sum, float* out, void* stream) {
  const int rc = lf_blend_check(pred, wgt, out, C, M, E);
  if (rc < 0) return rc;
  if (rc == 1) return 0;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (C % 4 == 0) && lf_al16(pred) && lf_al16(out);
  const int64_t width = sum ? C : 3 * (int64_t)C;
  const unsigned int total = (unsigned int)(M * width / (vec ? 4 : 1));
  const int blocks = dvgo_blocks(total, DVGO_BLOCK);
  if (vec && sum)
    liif_blend_fwd_kernel<4, true><<<blocks, DVGO_BLOCK, 0, st>>>(pred, wgt, C, M, E, total, out);
  else if (vec)
    liif_blend_fwd_kernel<4, false><<<blocks, DVGO_BLOCK, 0, st>>>(pred, wgt, C, M, E, total, out);
  else if (sum)
    liif_blend_fwd_kernel<1, true><<<blocks, DVGO_BLOCK, 0, st>>>(pred, wgt, C, M, E, total, out);
  else
    liif_blend_fwd_kernel<1, false><<<blocks, DVGO_BLOCK, 0, st>>>(pred, wgt, C, M, E, total, out);
  DVGO_LAUNCH_CHECK();
  return 0;
}

int dvgo_liif_blend_bwd(const float* grad_out, const float* wgt, int C, int64_t M, int E, int sum, float* grad_pred,
                        void* stream) {
  const int rc = lf_blend_check(grad_out, wgt, grad_pred, C, M, E);
  if (rc < 0) return rc;
  if (rc == 1) return 0;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (C % 4 == 0) && lf_al16(grad_out) && lf_al16(grad_pred);
  const unsigned int per = (unsigned int)(M * C / (vec ? 4 : 1));
  const dim3 grid((unsigned int)dvgo_blocks(per, DVGO_BLOCK), (unsigned int)(3 * E));
  if (vec)
    liif_blend_bwd_kernel<4><<<grid, DVGO_BLOCK, 0, st>>>(grad_out, wgt, C, M, E, sum, per, grad_pred);
  else
    liif_blend_bwd_kernel<1><<<grid, DVGO_BLOCK, 0, st>>>(grad_out, wgt, C, M, E, sum, per, grad_pred);
  DVGO_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
