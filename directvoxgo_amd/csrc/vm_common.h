// What the vector-matrix translation units share (vm.hip: the [M, 3R] feature sampler; vm_density.hip: the sampler
// that sums the 3R products on chip; march_vm.hip: the ray march over that sum, which uses the line descriptor and value,
// the pack of the line scalars and the vector-load predicate; vm_xyz.hip and march_raygrad.hip: the position derivative).
// Device: the line descriptor, the line value, the position derivative of planes times lines, the node-sum flush, one lane's walk of
// the gradient scatter and the scatter's kernel body (lane decode, the LDS table of mode 2).  Host: the pack of the 12 line
// scalars of an entry point, the vector-load predicate, the argument check and the launch shape of the scatter.
// include/dvgo_hip.h (the VM block) states the arithmetic.
#pragma once
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

// vm_line in two steps, for a caller that needs the node values as well as the line value (vm_xyz.hip): the same loads,
// in-range tests and fma chain as vm_line below, hence the same bits (vm_line itself stays as it is: DESIGN.md section 6o).
// VEC components from c on of the two nodes of the interval (n0, n0 + 1) of line q, and which nodes are in range: the
// loads come from clamped, always valid addresses, and a node out of range is dropped by whoever blends (zero padding)
template <int VEC>
struct VmNodes {
  bool ok0, ok1;
  TpVal<VEC> v0, v1;
};

template <int VEC>
__device__ __forceinline__ VmNodes<VEC> vm_gather(const VmLine& q, int c, int n0) {
  VmNodes<VEC> k;
  const int n1 = n0 + 1;
  k.ok0 = (n0 >= 0) & (n0 < q.N); k.ok1 = (n1 >= 0) & (n1 < q.N);
  const float* base = q.p + (int64_t)c * q.sC;
  k.v0 = tp_load<VEC>(base + (int64_t)min(max(n0, 0), q.N - 1) * q.sN, q.sC);
  k.v1 = tp_load<VEC>(base + (int64_t)min(max(n1, 0), q.N - 1) * q.sN, q.sC);
  return k;
}

// the line value of component i of the gathered nodes: the fma chain over the nodes from 0, nodes out of range skipped
template <int VEC>
__device__ __forceinline__ float vm_blend(const VmNodes<VEC>& k, int i, float w0, float w1) {
  float l = 0.f;
  l = k.ok0 ? fmaf(k.v0.v[i], w0, l) : l;
  l = k.ok1 ? fmaf(k.v1.v[i], w1, l) : l;
  return l;
}

// The incoming gradient of vm_xyz below, of components c .. c + VEC - 1 of plane s: `load` is issued with the group's
// gathers, ahead of the scheduling barrier, and `at` reads component c + i after it.
struct VmGradScalar {            // one gradient for all 3R products (the density: vm_xyz.hip, march_raygrad.hip)
  float g;
  struct Piece {};
  template <int VEC> __device__ __forceinline__ Piece load(int, int) const { return Piece{}; }
  __device__ __forceinline__ float at(const Piece&, int) const { return g; }
};

struct VmGradRow {               // the sample's row of grad_out [M, 3R] (the features: vm_xyz.hip)
  const float* __restrict__ row;
  int R;
  template <int VEC> __device__ __forceinline__ TpVal<VEC> load(int s, int c) const { return tp_load<VEC>(row + (int64_t)s * R + c, 1); }
  template <int VEC> __device__ __forceinline__ float at(const TpVal<VEC>& p, int i) const { return p.v[i]; }
};

// The position derivative of sum_{s,r} g_{s,r} * plane_{s,r}(p) * line_{s,r}(p) at p = (p[0], p[1], p[2]) in the box
// (mn, mx), added to (ox, oy, oz): per product g * l * (dp/dh, dp/dw) along the plane's two axes + g * p * dl/dn along the
// line's.  The cell, the node and the weights are the forward's (tp_setup, tp_axis on dvgo_src_index), and so are p and l
// (tp_blend, vm_blend on the corners and nodes of tp_gather, vm_gather); a corner or node the forward drops is dropped.
// Planes s = xy, yz, zx in turn, within a plane the components upwards, VEC at a time: the order of every sum.
template <int VEC, class Grad>
__device__ __forceinline__ void vm_xyz(const TpPlane& PA, const TpPlane& PB, const TpPlane& PC, const VmLine& LA, const VmLine& LB,
                                       const VmLine& LC, int R, const float (&p)[3], const float (&mn)[3], const float (&mx)[3],
                                       const Grad& grad, float& ox, float& oy, float& oz) {
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    int ah, aw, al;
    const TpPlane q = tp_pick(PA, PB, PC, s, ah, aw);
    const VmLine ln = vm_pick(LA, LB, LC, s, al);
    const BiSetup b = tp_setup(p[ah], p[aw], mn[ah], mx[ah], mn[aw], mx[aw], q.H, q.W);
    int n0;
    float w0, w1;
    tp_axis(dvgo_src_index(p[al], mn[al], mx[al], ln.N), n0, w0, w1);
    const float k00 = b.wh0 * b.ww0, k01 = b.wh0 * b.ww1, k10 = b.wh1 * b.ww0, k11 = b.wh1 * b.ww1;
    float Ah = 0.f, Aw = 0.f, An = 0.f;
    for (int c = 0; c < R; c += VEC) {
      const VmNodes<VEC> nd = vm_gather<VEC>(ln, c, n0);
      const TpCorners<VEC> k = tp_gather<VEC>(q, b, c);
      const auto gv = grad.template load<VEC>(s, c);
      // hipcc otherwise sinks each load to its first use (one round trip per corner); nothing crosses this
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const float l = vm_blend<VEC>(nd, i, w0, w1);
        const float pv = tp_blend<VEC>(k, i, k00, k01, k10, k11);
        float dh = 0.f, dw = 0.f;
        dh = (k.okh0 & k.okw0) ? fmaf(k.v00.v[i], -b.ww0, dh) : dh;
        dh = (k.okh0 & k.okw1) ? fmaf(k.v01.v[i], -b.ww1, dh) : dh;
        dh = (k.okh1 & k.okw0) ? fmaf(k.v10.v[i], b.ww0, dh) : dh;
        dh = (k.okh1 & k.okw1) ? fmaf(k.v11.v[i], b.ww1, dh) : dh;
        dw = (k.okh0 & k.okw0) ? fmaf(k.v00.v[i], -b.wh0, dw) : dw;
        dw = (k.okh0 & k.okw1) ? fmaf(k.v01.v[i], b.wh0, dw) : dw;
        dw = (k.okh1 & k.okw0) ? fmaf(k.v10.v[i], -b.wh1, dw) : dw;
        dw = (k.okh1 & k.okw1) ? fmaf(k.v11.v[i], b.wh1, dw) : dw;
        const float dn = (nd.ok1 ? nd.v1.v[i] : 0.f) - (nd.ok0 ? nd.v0.v[i] : 0.f);
        const float gi = grad.at(gv, i);
        const float t = gi * l, u = gi * pv;
        Ah = fmaf(t, dh, Ah);
        Aw = fmaf(t, dw, Aw);
        An = fmaf(u, dn, An);
      }
    }
    // the plane's scale once, after its last component; (ah, aw, al) is a permutation of the world axes
    const float th = Ah * ((float)(q.H - 1) / (mx[ah] - mn[ah]));
    const float tw = Aw * ((float)(q.W - 1) / (mx[aw] - mn[aw]));
    const float tn = An * ((float)(ln.N - 1) / (mx[al] - mn[al]));
    ox = ox + ((ah == 0) ? th : (aw == 0) ? tw : tn);
    oy = oy + ((ah == 1) ? th : (aw == 1) ? tw : tn);
    oz = oz + ((ah == 2) ? th : (aw == 2) ? tw : tn);
  }
}

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

// the two node sums of the interval (n0, n0 + 1) -> the line gradient (or the workgroup's table), nodes out of range dropped
__device__ __forceinline__ void vm_line_flush(float* __restrict__ base, int64_t sN, int N, int n0, float s0, float s1) {
  const int n1 = n0 + 1;
  if ((n0 >= 0) & (n0 < N)) atomicAdd(base + (int64_t)n0 * sN, s0);
  if ((n1 >= 0) & (n1 < N)) atomicAdd(base + (int64_t)n1 * sN, s1);
}

// One lane's walk: samples [chunk * run, min(+run, M)) of plane / line s, component r.  `lbase` / `lsN`: where the node
// sums go -- the line gradient of (s, r) with the line's node stride, or the table row of (s, r) with stride R.
// SKIP0: a sample whose incoming gradient is exactly 0 is passed over before anything else of it is read: it adds
// nothing, and the cell and the interval the lane is in stay what they were.
template <bool SKIP0>
__device__ __forceinline__ void vm_walk(const TpPlane& q, int ah, int aw, const VmLine& ln, int al, int r, float* __restrict__ gbase,
                                        float* __restrict__ lbase, int64_t lsN, const float* __restrict__ g, int64_t gstride,
                                        const float* __restrict__ xyz, const float* __restrict__ mn,
                                        const float* __restrict__ mx, int64_t m0, int64_t m1) {
  int ch = INT_MIN, cw = INT_MIN, cn = INT_MIN;
  float a00 = 0.f, a01 = 0.f, a10 = 0.f, a11 = 0.f, s0 = 0.f, s1 = 0.f;
  for (int64_t m = m0; m < m1; ++m) {
    float gv = 0.f;
    if constexpr (SKIP0) {
      gv = g[m * gstride];
      if (gv == 0.f) continue;
    }
    const BiSetup b = tp_setup(xyz, mn, mx, m, ah, aw, q.H, q.W);
    int n0;
    float w0, w1;
    tp_axis(dvgo_src_index(xyz[3 * m + al], mn[al], mx[al], ln.N), n0, w0, w1);
    const float l = vm_line<1>(ln, r, n0, w0, w1).v[0];
    const float p = tp_sample<1>(q, ah, aw, r, xyz, mn, mx, m).v[0];
    if constexpr (!SKIP0) gv = g[m * gstride];
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

// The body of a scatter kernel.  total = nchunk * 3R lanes, nchunk = ceil(M / run); workgroup b walks the lanes
// [b * share, (b + 1) * share), share a multiple of the workgroup size (mode 1: the workgroup size itself).  CFAST:
// component fastest, else sample fastest.  LDS: the node sums go through the table `tab` [Na + Nb + Nc][R] (dynamic LDS).
// The lane of (s, r) reads its incoming gradient at grad_out[s * goff_s + r + m * gstride] when PER_COMP ([M, 3R]: R, 3R)
// and at grad_out[m] otherwise, where it also passes over exact zeros (vm_walk's SKIP0).
template <bool CFAST, bool LDS, bool PER_COMP>
__device__ __forceinline__ void vm_scatter_body(float* tab, TpPlane PA, TpPlane PB, TpPlane PC, VmLine LA, VmLine LB, VmLine LC,
                                                VmGrads GP, VmGrads GL, int R, const float* __restrict__ grad_out,
                                                const float* __restrict__ xyz, const float* __restrict__ mn,
                                                const float* __restrict__ mx, int64_t M, int run, int64_t nchunk,
                                                int64_t total, int64_t share) {
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
    if constexpr (PER_COMP)
      vm_walk<false>(q, ah, aw, ln, al, r, gbase, lbase, lsN, grad_out + (int64_t)s * R + r, 3 * (int64_t)R, xyz, mn, mx, m0, m1);
    else
      vm_walk<true>(q, ah, aw, ln, al, r, gbase, lbase, lsN, grad_out, 1, xyz, mn, mx, m0, m1);
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

// ---------------------------------------------------------------------------------------------- host side
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

// the same for an entry with an incoming gradient `in` and an output `out` (vm_xyz.hip)
static int vm_check(const TpPlanes& P, const VmLines& L, int R, int64_t M, const void* xyz, const void* mn, const void* mx,
                    const void* in, const void* out) {
  return tp_check(P, R, M, L.a.N >= 1 && L.b.N >= 1 && L.c.N >= 1, xyz, mn, mx, {L.a.p, L.b.p, L.c.p, in, out}, 3, R);
}

// The argument check and the launch shape of a scatter entry, after `vm_check` semantics: < 0 the error, 1 nothing to do,
// 0 launch with what `S` holds.  `io`: the incoming gradient.
struct VmScatter {
  TpScatter S;
  int mode;
  bool cfast;
  int64_t blocks, share;
  size_t tab_bytes;
};

static int vm_scatter(const TpPlanes& P, const VmLines& L, int R, int64_t M, const void* xyz, const void* mn, const void* mx,
                      const void* io, const VmGrads& GP, const VmGrads& GL, int run, int mode, VmScatter& V) {
  if (run < 0 || mode < 0 || mode > 2) return DVGO_EINVAL;
  const int rc = vm_check(P, L, R, M, xyz, mn, mx, io);
  if (rc) return rc;
  if (!GP.a || !GP.b || !GP.c || !GL.a || !GL.b || !GL.c) return DVGO_EINVAL;
  const int64_t tab_bytes = ((int64_t)L.a.N + L.b.N + L.c.N) * R * (int64_t)sizeof(float);
  if (mode == 2 && tab_bytes > VM_LDS_BYTES) return DVGO_EINVAL;
  if (mode == 0) mode = (VM_MODE_DEFAULT == 2 && tab_bytes <= VM_LDS_BYTES) ? 2 : 1;
  V.S = tp_scatter(P, R, M, run, VM_RUN_DEFAULT, 3 * R);
  V.mode = mode;
  V.cfast = V.S.cfast && L.a.sC == 1 && L.b.sC == 1 && L.c.sC == 1;          // the lines channels-last as well
  V.blocks = dvgo_blocks(V.S.lanes, DVGO_BLOCK);
  V.share = DVGO_BLOCK;
  if (mode == 2 && V.blocks > VM_LDS_GRID) {
    V.share = ((V.blocks + VM_LDS_GRID - 1) / VM_LDS_GRID) * DVGO_BLOCK;
    V.blocks = (V.S.lanes + V.share - 1) / V.share;
  }
  V.tab_bytes = (mode == 2) ? (size_t)tab_bytes : 0;
  return 0;
}
