// Vector-matrix (VM) decomposed density (TensoRF, Chen et al., ECCV 2022): the 3R products plane value times line value of
// vm.hip summed into one float per sample on chip, and the gradient scatter of that sum into planes and lines.
// include/dvgo_hip.h (the VM density block) states the arithmetic; p and l are vm.hip's, through plane2d.h and vm_common.h,
// bit for bit.  No [M, 3R] intermediate exists anywhere: the forward keeps one accumulator per sample in a register, the
// backward reads one float of incoming gradient per sample.
//
// Forward: a lane owns one sample and walks s = xy, yz, zx and, within a plane, the components upwards, VEC at a time:
// acc = fmaf(p, l, acc) from acc = 0.  That order is the contract, the same for VEC = 4 and VEC = 1, so the result does
// not depend on the layout.  What is left to write is 4 bytes per sample; the kernel is bound by its gathers, 3 * (4
// corners + 2 nodes) per component (group), which hit L2 or the vector cache: planes and lines are a few MB, and the
// lanes of a wave are consecutive samples of a ray, which share texels.  The coordinate arithmetic of a plane (two
// divisions per axis) is loop invariant and hoisted out of the component loop by the compiler.
// VEC = 4 needs R % 4 == 0 and channels-last, 16-byte aligned planes and lines; VEC = 1 is everything else.
//
// Backward: vm.hip's scatter (vm_common.h: lane = (run of samples, plane s, component r), corner and node sums in
// registers, modes 1 and 2) with the incoming gradient read at grad_out[m] by all 3R lanes of a sample -- one address per
// wave instruction when the component runs fastest -- and a sample whose gradient is exactly 0 passed over before its
// position is even read: it issues no atomic and does not end the run of the cell the lane is in.
#include "vm_common.h"

// total = M lanes
template <int VEC>
__global__ void __launch_bounds__(DVGO_BLOCK)
vmd_fwd_kernel(TpPlane PA, TpPlane PB, TpPlane PC, VmLine LA, VmLine LB, VmLine LC, int R, const float* __restrict__ xyz,
               const float* __restrict__ mn, const float* __restrict__ mx, int64_t M, float* __restrict__ out) {
  const int64_t m = (int64_t)blockIdx.x * DVGO_BLOCK + threadIdx.x;
  if (m >= M) return;
  float acc = 0.f;
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    int ah, aw, al;
    const TpPlane q = tp_pick(PA, PB, PC, s, ah, aw);
    const VmLine ln = vm_pick(LA, LB, LC, s, al);
    int n0;
    float w0, w1;
    tp_axis(dvgo_src_index(xyz[3 * m + al], mn[al], mx[al], ln.N), n0, w0, w1);
#pragma unroll 2
    for (int c = 0; c < R; c += VEC) {
      const TpVal<VEC> l = vm_line<VEC>(ln, c, n0, w0, w1);
      const TpVal<VEC> p = tp_sample<VEC>(q, ah, aw, c, xyz, mn, mx, m);
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc = fmaf(p.v[i], l.v[i], acc);
    }
  }
  out[m] = acc;
}

// vm_bwd_kernel's launch shape; the lanes read grad_out[m]
template <bool CFAST, bool LDS>
__global__ void __launch_bounds__(DVGO_BLOCK)
vmd_bwd_kernel(TpPlane PA, TpPlane PB, TpPlane PC, VmLine LA, VmLine LB, VmLine LC, VmGrads GP, VmGrads GL, int R,
               const float* __restrict__ grad_out, const float* __restrict__ xyz, const float* __restrict__ mn,
               const float* __restrict__ mx, int64_t M, int run, int64_t nchunk, int64_t total, int64_t share) {
  extern __shared__ float tab[];
  vm_scatter_body<CFAST, LDS, false>(tab, PA, PB, PC, LA, LB, LC, GP, GL, R, grad_out, xyz, mn, mx, M, run, nchunk, total, share);
}

extern "C" {

int dvgo_vm_density_fwd(const float* xy, int H_xy, int W_xy, int64_t sC_xy, int64_t sH_xy, int64_t sW_xy,
                        const float* yz, int H_yz, int W_yz, int64_t sC_yz, int64_t sH_yz, int64_t sW_yz,
                        const float* zx, int H_zx, int W_zx, int64_t sC_zx, int64_t sH_zx, int64_t sW_zx,
                        const float* l_xy, int N_xy, int64_t lC_xy, int64_t lN_xy,
                        const float* l_yz, int N_yz, int64_t lC_yz, int64_t lN_yz,
                        const float* l_zx, int N_zx, int64_t lC_zx, int64_t lN_zx,
                        int R, const float* xyz, const float* xyz_min, const float* xyz_max, int64_t M, float* out,
                        void* stream) {
  const TpPlanes P = TP_PLANES(xy, yz, zx);
  const VmLines L = VM_LINES();
  const int rc = vm_check(P, L, R, M, xyz, xyz_min, xyz_max, out);
  if (rc) return rc < 0 ? rc : 0;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (R % 4 == 0) && tp_planes_vec(P, 4) && vm_line_vec(L.a) && vm_line_vec(L.b) && vm_line_vec(L.c);
  const int blocks = dvgo_blocks(M, DVGO_BLOCK);
  if (vec)
    vmd_fwd_kernel<4><<<blocks, DVGO_BLOCK, 0, st>>>(P.a, P.b, P.c, L.a, L.b, L.c, R, xyz, xyz_min, xyz_max, M, out);
  else
    vmd_fwd_kernel<1><<<blocks, DVGO_BLOCK, 0, st>>>(P.a, P.b, P.c, L.a, L.b, L.c, R, xyz, xyz_min, xyz_max, M, out);
  DVGO_LAUNCH_CHECK();
  return 0;
}

int dvgo_vm_density_bwd(const float* grad_out,
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
#define VMD_LAUNCH(CF, LDS)                                                                                                  \
  vmd_bwd_kernel<CF, LDS><<<(int)V.blocks, DVGO_BLOCK, V.tab_bytes, st>>>(P.a, P.b, P.c, L.a, L.b, L.c, GP, GL, R, grad_out, \
                                                                          xyz, xyz_min, xyz_max, M, V.S.run, V.S.nchunk,     \
                                                                          V.S.lanes, V.share)
  if (V.mode == 2) {
    if (V.cfast) VMD_LAUNCH(true, true); else VMD_LAUNCH(false, true);
  } else {
    if (V.cfast) VMD_LAUNCH(true, false); else VMD_LAUNCH(false, false);
  }
#undef VMD_LAUNCH
  DVGO_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
