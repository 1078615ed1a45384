// Vector-matrix (VM) decomposed features (TensoRF, Chen et al., ECCV 2022): three 2-D planes, each multiplied component
// by component by a 1-D line along the world axis its plane does not see, the products concatenated; and the gradient
// scatter into planes and lines.  include/dvgo_hip.h (the VM block) states the arithmetic; the plane half is
// triplane.hip's, through plane2d.h, so a plane value carries the bits of dvgo_triplane_fwd's 'concat' output.
//
// Forward: bound by its output write ([M, 3R] floats), like triplane_fwd_kernel, and laid out like it: a lane owns VEC
// consecutive components of one output row, (sample, plane, component group); a wave's stores are 64 consecutive pieces
// of `out`.  The four corner loads and the two node loads are unconditional (a corner or node out of range reads a
// clamped, valid address and is dropped by a select), so the six are in flight together; the fma chains run afterwards.
// VEC = 4 needs R % 4 == 0 and channels-last, 16-byte aligned planes, lines and out; VEC = 1 is everything else.
//
// Backward: a sample's component (s, r) adds into four texels and two line nodes: 3R * 6 atomic dwords per sample when
// nothing is merged.  A lane owns (a run of consecutive samples, plane s, component r), recomputes the plane value p and
// the line value l per sample (planes and lines are a few MB: L2), keeps the four corner sums of the texel cell it is
// in and, independently, the two node sums of the line interval it is in, in registers, and issues its atomics when the
// cell (the interval) changes and at the end of its run.  Lane order as in triplane_bwd_kernel: component fastest when
// everything is channels-last, sample fastest otherwise.
//   mode 1  all six sums go to global memory.  Every shape.
//   mode 2  the node sums go to a table [3][N_s][R] in LDS; a workgroup walks a contiguous share of the lanes (the grid is
//           capped so that a share is long) and adds its table to the line gradients once, component fastest -- a
//           wave-instruction adds contiguous runs when the lines are channels-last -- skipping entries that are zero.
//           Legal while the table is at most 64 KB.
#include "common.h"
#include "plane2d.h"

// mode 0's choice and the run length a lane merges by default, from the A/B of profiles/vm/README.md: at R = 16, planes
// 160^2, lines 160 and 2 097 152 samples mode 2 took 0.86 ms against mode 1's 1.31 ms, both at run 8, the best run of
// {1, 2, 4, 8} in every case measured.  Where mode 2's table does not fit, mode 0 is mode 1.
#define VM_MODE_DEFAULT 2
#define VM_RUN_DEFAULT 8
#define VM_LDS_BYTES (64 * 1024)
// workgroups of a mode-2 launch at the most: each adds its whole table once
#define VM_LDS_GRID 1024

struct VmLine {
  float* p;
  int N;
  int64_t sC, sN;
};

struct VmGrads { float *a, *b, *c; };

// line s of the three and the world axis it follows: the one plane s does not see
__device__ __forceinline__ VmLine vm_pick(const VmLine A, const VmLine B, const VmLine D, int s, int& al) {
  al = (s == 0) ? 0 : (s == 1) ? 2 : 1;
  VmLine q;
  q.p = (s == 0) ? A.p : (s == 1) ? B.p : D.p;
  q.N = (s == 0) ? A.N : (s == 1) ? B.N : D.N;
  q.sC = (s == 0) ? A.sC : (s == 1) ? B.sC : D.sC;
  q.sN = (s == 0) ? A.sN : (s == 1) ? B.sN : D.sN;
  return q;
}

__device__ __forceinline__ float* vm_pick(const VmGrads G, int s) { return (s == 0) ? G.a : (s == 1) ? G.b : G.c; }

// VEC components from c on of line q in the interval (n0, n0 + 1) with the weights (w0, w1)
template <int VEC>
__device__ __forceinline__ TpVal<VEC> vm_line(const VmLine& q, int c, int n0, float w0, float w1) {
  const int n1 = n0 + 1;
  const bool ok0 = (n0 >= 0) & (n0 < q.N), ok1 = (n1 >= 0) & (n1 < q.N);
  const float* base = q.p + (int64_t)c * q.sC;
  const TpVal<VEC> v0 = tp_load<VEC>(base + (int64_t)min(max(n0, 0), q.N - 1) * q.sN, q.sC);
  const TpVal<VEC> v1 = tp_load<VEC>(base + (int64_t)min(max(n1, 0), q.N - 1) * q.sN, q.sC);
  TpVal<VEC> r;
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    float l = 0.f;
    l = ok0 ? fmaf(v0.v[i], w0, l) : l;
    l = ok1 ? fmaf(v1.v[i], w1, l) : l;
    r.v[i] = l;
  }
  return r;
}

// total = M * 3R / VEC lanes (< 2^31: the entry checks M * 3R)
template <int VEC>
__global__ void __launch_bounds__(DVGO_BLOCK)
vm_fwd_kernel(TpPlane PA, TpPlane PB, TpPlane PC, VmLine LA, VmLine LB, VmLine LC, int R, const float* __restrict__ xyz,
              const float* __restrict__ mn, const float* __restrict__ mx, unsigned int total, float* __restrict__ out) {
  const unsigned int tid = blockIdx.x * (unsigned int)DVGO_BLOCK + threadIdx.x;
  if (tid >= total) return;
  const unsigned int cg = (unsigned int)R / VEC;         // component groups of a plane
  const unsigned int per = 3u * cg;                      // lanes of a sample
  const unsigned int m = tid / per, j = tid - m * per;
  const unsigned int s = j / cg;
  const int c = (int)(j - s * cg) * VEC;
  int ah, aw, al;
  const TpPlane q = tp_pick(PA, PB, PC, (int)s, ah, aw);
  const VmLine ln = vm_pick(LA, LB, LC, (int)s, al);
  int n0;
  float w0, w1;
  tp_axis(dvgo_src_index(xyz[3 * (int64_t)m + al], mn[al], mx[al], ln.N), n0, w0, w1);
  const TpVal<VEC> l = vm_line<VEC>(ln, c, n0, w0, w1);
  const TpVal<VEC> p = tp_sample<VEC>(q, ah, aw, c, xyz, mn, mx, m);
  float* o = out + (int64_t)tid * VEC;
  if constexpr (VEC == 4) {
    *reinterpret_cast<float4*>(o) = make_float4(p.v[0] * l.v[0], p.v[1] * l.v[1], p.v[2] * l.v[2], p.v[3] * l.v[3]);
  } else {
#pragma unroll
    for (int i = 0; i < VEC; ++i) o[i] = p.v[i] * l.v[i];
  }
}

// the two node sums of the interval (n0, n0 + 1) -> the line gradient (or the workgroup's table), nodes out of range dropped
__device__ __forceinline__ void vm_line_flush(float* __restrict__ base, int64_t sN, int N, int n0, float s0, float s1) {
  const int n1 = n0 + 1;
  if ((n0 >= 0) & (n0 < N)) atomicAdd(base + (int64_t)n0 * sN, s0);
  if ((n1 >= 0) & (n1 < N)) atomicAdd(base + (int64_t)n1 * sN, s1);
}

// One lane's walk: samples [chunk * run, min(+run, M)) of plane / line s, component r.  `lbase` / `lsN`: where the node
// sums go -- the line gradient of (s, r) with the line's node stride, or the table row of (s, r) with stride R.
__device__ __forceinline__ void vm_walk(const TpPlane& q, int ah, int aw, const VmLine& ln, int al, int r, float* __restrict__ gbase,
                                        float* __restrict__ lbase, int64_t lsN, const float* __restrict__ g, int64_t gstride,
                                        const float* __restrict__ xyz, const float* __restrict__ mn,
                                        const float* __restrict__ mx, int64_t m0, int64_t m1) {
  int ch = INT_MIN, cw = INT_MIN, cn = INT_MIN;
  float a00 = 0.f, a01 = 0.f, a10 = 0.f, a11 = 0.f, s0 = 0.f, s1 = 0.f;
  for (int64_t m = m0; m < m1; ++m) {
    const BiSetup b = tp_setup(xyz, mn, mx, m, ah, aw, q.H, q.W);
    int n0;
    float w0, w1;
    tp_axis(dvgo_src_index(xyz[3 * m + al], mn[al], mx[al], ln.N), n0, w0, w1);
    const float l = vm_line<1>(ln, r, n0, w0, w1).v[0];
    const float p = tp_sample<1>(q, ah, aw, r, xyz, mn, mx, m).v[0];
    const float gv = g[m * gstride];
    if ((b.h0 != ch) | (b.w0 != cw)) {
      if (ch != INT_MIN) tp_flush(q, gbase, ch, cw, a00, a01, a10, a11);
      ch = b.h0; cw = b.w0;
      a00 = a01 = a10 = a11 = 0.f;
    }
    if (n0 != cn) {
      if (cn != INT_MIN) vm_line_flush(lbase, lsN, ln.N, cn, s0, s1);
      cn = n0;
      s0 = s1 = 0.f;
    }
    const float tl = l * gv, tp = p * gv;
    a00 += (b.wh0 * b.ww0) * tl;
    a01 += (b.wh0 * b.ww1) * tl;
    a10 += (b.wh1 * b.ww0) * tl;
    a11 += (b.wh1 * b.ww1) * tl;
    s0 += w0 * tp;
    s1 += w1 * tp;
  }
  if (ch != INT_MIN) tp_flush(q, gbase, ch, cw, a00, a01, a10, a11);
  if (cn != INT_MIN) vm_line_flush(lbase, lsN, ln.N, cn, s0, s1);
}

// total = nchunk * 3R lanes, nchunk = ceil(M / run); workgroup b walks the lanes [b * share, (b + 1) * share), share a
// multiple of the workgroup size (mode 1: the workgroup size itself).  CFAST: component fastest, else sample fastest.
// LDS: the node sums go through the table `tab` [Na + Nb + Nc][R] (dynamic LDS).
template <bool CFAST, bool LDS>
__global__ void __launch_bounds__(DVGO_BLOCK)
vm_bwd_kernel(TpPlane PA, TpPlane PB, TpPlane PC, VmLine LA, VmLine LB, VmLine LC, VmGrads GP, VmGrads GL, int R,
              const float* __restrict__ grad_out, const float* __restrict__ xyz, const float* __restrict__ mn,
              const float* __restrict__ mx, int64_t M, int run, int64_t nchunk, int64_t total, int64_t share) {
  extern __shared__ float tab[];
  const int rows = LA.N + LB.N + LC.N;
  if (LDS) {
    for (int i = threadIdx.x; i < rows * R; i += DVGO_BLOCK) tab[i] = 0.f;
    __syncthreads();
  }
  const int64_t first = (int64_t)blockIdx.x * share;
  const int64_t last = (first + share < total) ? first + share : total;
  for (int64_t tid = first + threadIdx.x; tid < last; tid += DVGO_BLOCK) {
    int64_t chunk;
    int s, r;
    if (CFAST) {
      chunk = tid / (3 * R);
      const int j = (int)(tid - chunk * (3 * R));
      s = j / R;
      r = j - s * R;
    } else {
      const int sr = (int)(tid / nchunk);
      chunk = tid - (int64_t)sr * nchunk;
      s = sr / R;
      r = sr - s * R;
    }
    int ah, aw, al;
    const TpPlane q = tp_pick(PA, PB, PC, s, ah, aw);
    const VmLine ln = vm_pick(LA, LB, LC, s, al);
    float* gbase = vm_pick(GP, s) + (int64_t)r * q.sC;
    float* lbase;
    int64_t lsN;
    if (LDS) {
      const int row0 = (s == 0) ? 0 : (s == 1) ? LA.N : LA.N + LB.N;
      lbase = tab + row0 * R + r;
      lsN = R;
    } else {
      lbase = vm_pick(GL, s) + (int64_t)r * ln.sC;
      lsN = ln.sN;
    }
    const int64_t m0 = chunk * run;
    const int64_t m1 = (m0 + run < M) ? m0 + run : M;
    vm_walk(q, ah, aw, ln, al, r, gbase, lbase, lsN, grad_out + (int64_t)s * R + r, 3 * (int64_t)R, xyz, mn, mx, m0, m1);
  }
  if (LDS) {
    __syncthreads();
    for (int i = threadIdx.x; i < rows * R; i += DVGO_BLOCK) {
      const float v = tab[i];
      if (v == 0.f) continue;
      const int row = i / R, r = i - row * R;
      const int s = (row < LA.N) ? 0 : (row < LA.N + LB.N) ? 1 : 2;
      const int n = row - ((s == 0) ? 0 : (s == 1) ? LA.N : LA.N + LB.N);
      int al;
      const VmLine ln = vm_pick(LA, LB, LC, s, al);
      atomicAdd(vm_pick(GL, s) + (int64_t)r * ln.sC + (int64_t)n * ln.sN, v);
    }
  }
}

static bool vm_line_vec(const VmLine& q) { return q.sC == 1 && (q.sN % 4 == 0 || q.N == 1) && ((((uintptr_t)q.p) & 15) == 0); }

struct VmLines { VmLine a, b, c; };

// the three lines of an entry point from its 12 line scalars
#define VM_LINES()                                                      \
  VmLines{VmLine{const_cast<float*>(l_xy), N_xy, lC_xy, lN_xy},         \
          VmLine{const_cast<float*>(l_yz), N_yz, lC_yz, lN_yz},         \
          VmLine{const_cast<float*>(l_zx), N_zx, lC_zx, lN_zx}}

// tp_check with the lines' lengths among the shapes and their pointers among the pointers
static int vm_check(const TpPlanes& P, const VmLines& L, int R, int64_t M, const void* xyz, const void* mn, const void* mx,
                    const void* io) {
  return tp_check(P, R, M, L.a.N >= 1 && L.b.N >= 1 && L.c.N >= 1, xyz, mn, mx, {L.a.p, L.b.p, L.c.p, io}, 3, R);
}

extern "C" {

int dvgo_vm_fwd(const float* xy, int H_xy, int W_xy, int64_t sC_xy, int64_t sH_xy, int64_t sW_xy,
                const float* yz, int H_yz, int W_yz, int64_t sC_yz, int64_t sH_yz, int64_t sW_yz,
                const float* zx, int H_zx, int W_zx, int64_t sC_zx, int64_t sH_zx, int64_t sW_zx,
                const float* l_xy, int N_xy, int64_t lC_xy, int64_t lN_xy,
                const float* l_yz, int N_yz, int64_t lC_yz, int64_t lN_yz,
                const float* l_zx, int N_zx, int64_t lC_zx, int64_t lN_zx,
                int R, const float* xyz, const float* xyz_min, const float* xyz_max, int64_t M, float* out, void* stream) {
  const TpPlanes P = TP_PLANES(xy, yz, zx);
  const VmLines L = VM_LINES();
  const int rc = vm_check(P, L, R, M, xyz, xyz_min, xyz_max, out);
  if (rc) return rc < 0 ? rc : 0;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (R % 4 == 0) && tp_planes_vec(P, 4) && vm_line_vec(L.a) && vm_line_vec(L.b) && vm_line_vec(L.c) &&
                   ((((uintptr_t)out) & 15) == 0);
  const unsigned int total = (unsigned int)(M * 3 * (int64_t)R / (vec ? 4 : 1));
  const int blocks = dvgo_blocks(total, DVGO_BLOCK);
  if (vec)
    vm_fwd_kernel<4><<<blocks, DVGO_BLOCK, 0, st>>>(P.a, P.b, P.c, L.a, L.b, L.c, R, xyz, xyz_min, xyz_max, total, out);
  else
    vm_fwd_kernel<1><<<blocks, DVGO_BLOCK, 0, st>>>(P.a, P.b, P.c, L.a, L.b, L.c, R, xyz, xyz_min, xyz_max, total, out);
  DVGO_LAUNCH_CHECK();
  return 0;
}

int dvgo_vm_bwd(const float* grad_out,
                const float* xy, int H_xy, int W_xy, int64_t sC_xy, int64_t sH_xy, int64_t sW_xy,
                const float* yz, int H_yz, int W_yz, int64_t sC_yz, int64_t sH_yz, int64_t sW_yz,
                const float* zx, int H_zx, int W_zx, int64_t sC_zx, int64_t sH_zx, int64_t sW_zx,
                const float* l_xy, int N_xy, int64_t lC_xy, int64_t lN_xy,
                const float* l_yz, int N_yz, int64_t lC_yz, int64_t lN_yz,
                const float* l_zx, int N_zx, int64_t lC_zx, int64_t lN_zx,
                float* g_xy, float* g_yz, float* g_zx, float* gl_xy, float* gl_yz, float* gl_zx,
                int R, const float* xyz, const float* xyz_min, const float* xyz_max, int64_t M, int run, int mode,
                void* stream) {
  const TpPlanes P = TP_PLANES(xy, yz, zx);
  const VmLines L = VM_LINES();
  if (run < 0 || mode < 0 || mode > 2) return DVGO_EINVAL;
  const int rc = vm_check(P, L, R, M, xyz, xyz_min, xyz_max, grad_out);
  if (rc) return rc < 0 ? rc : 0;
  if (!g_xy || !g_yz || !g_zx || !gl_xy || !gl_yz || !gl_zx) return DVGO_EINVAL;
  const int64_t tab_bytes = ((int64_t)N_xy + N_yz + N_zx) * R * (int64_t)sizeof(float);
  if (mode == 2 && tab_bytes > VM_LDS_BYTES) return DVGO_EINVAL;
  if (mode == 0) mode = (VM_MODE_DEFAULT == 2 && tab_bytes <= VM_LDS_BYTES) ? 2 : 1;
  hipStream_t st = (hipStream_t)stream;
  const TpScatter S = tp_scatter(P, R, M, run, VM_RUN_DEFAULT, 3 * R);
  const VmGrads GP{g_xy, g_yz, g_zx}, GL{gl_xy, gl_yz, gl_zx};
  const bool cfast = S.cfast && L.a.sC == 1 && L.b.sC == 1 && L.c.sC == 1;          // the lines channels-last as well
  int64_t blocks = dvgo_blocks(S.lanes, DVGO_BLOCK), share = DVGO_BLOCK;
  if (mode == 2 && blocks > VM_LDS_GRID) {
    share = ((blocks + VM_LDS_GRID - 1) / VM_LDS_GRID) * DVGO_BLOCK;
    blocks = (S.lanes + share - 1) / share;
  }
#define VM_LAUNCH(CF, LDS, bytes)                                                                                          \
  vm_bwd_kernel<CF, LDS><<<(int)blocks, DVGO_BLOCK, bytes, st>>>(P.a, P.b, P.c, L.a, L.b, L.c, GP, GL, R, grad_out, xyz,   \
                                                                 xyz_min, xyz_max, M, S.run, S.nchunk, S.lanes, share)
  if (mode == 2) {
    if (cfast) VM_LAUNCH(true, true, (size_t)tab_bytes); else VM_LAUNCH(false, true, (size_t)tab_bytes);
  } else {
    if (cfast) VM_LAUNCH(true, false, 0); else VM_LAUNCH(false, false, 0);
  }
#undef VM_LAUNCH
  DVGO_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
