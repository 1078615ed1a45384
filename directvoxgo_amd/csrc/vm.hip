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
//
// The line arithmetic, a lane's walk, the scatter's body and the entry checks live in vm_common.h, which vm_density.hip
// shares.
#include "vm_common.h"

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

// total = nchunk * 3R lanes, nchunk = ceil(M / run); workgroup b walks the lanes [b * share, (b + 1) * share), share a
// multiple of the workgroup size (mode 1: the workgroup size itself).  CFAST: component fastest, else sample fastest.
// LDS: the node sums go through the table `tab` [Na + Nb + Nc][R] (dynamic LDS).
template <bool CFAST, bool LDS>
__global__ void __launch_bounds__(DVGO_BLOCK)
vm_bwd_kernel(TpPlane PA, TpPlane PB, TpPlane PC, VmLine LA, VmLine LB, VmLine LC, VmGrads GP, VmGrads GL, int R,
              const float* __restrict__ grad_out, const float* __restrict__ xyz, const float* __restrict__ mn,
              const float* __restrict__ mx, int64_t M, int run, int64_t nchunk, int64_t total, int64_t share) {
  extern __shared__ float tab[];
  vm_scatter_body<CFAST, LDS, true>(tab, PA, PB, PC, LA, LB, LC, GP, GL, R, grad_out, xyz, mn, mx, M, run, nchunk, total, share);
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
  const VmGrads GP{g_xy, g_yz, g_zx}, GL{gl_xy, gl_yz, gl_zx};
  VmScatter V;
  const int rc = vm_scatter(P, L, R, M, xyz, xyz_min, xyz_max, grad_out, GP, GL, run, mode, V);
  if (rc) return rc < 0 ? rc : 0;
  hipStream_t st = (hipStream_t)stream;
#define VM_LAUNCH(CF, LDS)                                                                                                  \
  vm_bwd_kernel<CF, LDS><<<(int)V.blocks, DVGO_BLOCK, V.tab_bytes, st>>>(P.a, P.b, P.c, L.a, L.b, L.c, GP, GL, R, grad_out, \
                                                                         xyz, xyz_min, xyz_max, M, V.S.run, V.S.nchunk,     \
                                                                         V.S.lanes, V.share)
  if (V.mode == 2) {
    if (V.cfast) VM_LAUNCH(true, true); else VM_LAUNCH(false, true);
  } else {
    if (V.cfast) VM_LAUNCH(true, false); else VM_LAUNCH(false, false);
  }
#undef VM_LAUNCH
  DVGO_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
