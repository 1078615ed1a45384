// Gradient of the vector-matrix (VM) samplers with respect to the sample POSITION: what camera-pose refinement
// differentiates through when the colour features (vm.hip, [M, 3R]) or the density (vm_density.hip, [M]) come from planes
// times lines (ops.vm_sample / ops.vm_density with position_grad=True, VMTriPlaneVoxGO / TensoRFVoxGO with raygrad=True,
// pose.py).  The gradients of planes and lines are the scatters of vm.hip and vm_density.hip.  include/dvgo_hip.h (the VM
// block) states the arithmetic.
//
// One kernel body, two entries: the incoming gradient of component (s, r) is grad_out[m, sR + r] for the features and
// grad_out[m] for the density.  The derivative itself is vm_common.h's vm_xyz, which march_raygrad.hip's VM kernel calls per
// record of a ray; what follows describes it as this unit runs it.  Both are sums over the 3R products of
//     g * d(p * l)/dxyz = g * l * (dp/dh, dp/dw) along the plane's two axes  +  g * p * dl/dn along the line's axis.
//
// One lane per sample, as in vmd_fwd_kernel and hash_xyz.hip: the lane walks s = xy, yz, zx and, within a plane, the
// components upwards, VEC at a time.  The cell, the node and the weights are the forward's (tp_setup, tp_axis on
// dvgo_src_index: same expressions, same bits), and so are p and l (tp_blend, vm_blend on the corners and nodes of
// tp_gather, vm_gather: the forward's loads and fma chains), so the derivative is that of the cell the forward chose.  The
// forward zero-pads -- a corner or node out of range is dropped, the weights are not clamped -- and the derivative drops
// the same corners and nodes: less than one cell outside the box it is not zero; further out, or at a NaN coordinate, every
// term is dropped and the row is exactly 0.0.  Every row of grad_xyz is written by its lane with plain stores: no atomics,
// no workspace, nothing to zero beforehand, and the order of every sum is the loops', whatever VEC and the layout.
//
// Why this mapping and not the scatters' (run of samples, plane, component) lanes.  The three outputs of a sample are sums
// over its 3R components and have to come out in one fixed order; with a lane per (sample, s, r) that is a reduction over
// 3R lanes, 3R being any number, which straddle waves: LDS and a barrier, or atomics on grad_xyz and a zero fill, to add
// 3R numbers.  Here the sums are registers and their order is the loop's.  What the kernel costs is its gathers, the
// forward's own: 4 corners + 2 nodes per plane and component group, from always valid (clamped) addresses, issued ahead of
// the first fmaf of the group; planes and lines are a few MB and the lanes of a wave are consecutive samples of a ray, so
// they hit L2 or the vector cache.  The feature entry also reads its grad_out piece, 4 VEC bytes at a stride of 12 R bytes
// from its neighbour's; the pieces of a sample are consecutive, so a line fetched for one group serves the groups after it.
// The plane and the line of s are selected from by-value kernel arguments (tp_pick, vm_pick): no private memory.
// VEC = 4 needs R % 4 == 0 and channels-last, 16-byte aligned planes and lines (the feature entry: grad_out as well);
// VEC = 1 is everything else.
#include "vm_common.h"

// total = M lanes.  PER_COMP: grad_out [M, 3R], else grad_out [M], where a sample whose gradient is exactly 0 is passed over
template <int VEC, bool PER_COMP>
__global__ void __launch_bounds__(DVGO_BLOCK)
vm_bwd_xyz_kernel(TpPlane PA, TpPlane PB, TpPlane PC, VmLine LA, VmLine LB, VmLine LC, int R,
                  const float* __restrict__ grad_out, const float* __restrict__ xyz, const float* __restrict__ mn,
                  const float* __restrict__ mx, int64_t M, float* __restrict__ grad_xyz) {
  const int64_t m = (int64_t)blockIdx.x * DVGO_BLOCK + threadIdx.x;
  if (m >= M) return;
  float ox = 0.f, oy = 0.f, oz = 0.f;
  float gd = 0.f;
  if constexpr (!PER_COMP) {
    gd = grad_out[m];
    if (gd == 0.f) {
      grad_xyz[3 * m + 0] = ox;
      grad_xyz[3 * m + 1] = oy;
      grad_xyz[3 * m + 2] = oz;
      return;
    }
  }
  const float p[3] = {xyz[3 * m], xyz[3 * m + 1], xyz[3 * m + 2]};
  const float lo[3] = {mn[0], mn[1], mn[2]}, hi[3] = {mx[0], mx[1], mx[2]};
  if constexpr (PER_COMP)
    vm_xyz<VEC>(PA, PB, PC, LA, LB, LC, R, p, lo, hi, VmGradRow{grad_out + m * (3 * (int64_t)R), R}, ox, oy, oz);
  else
    vm_xyz<VEC>(PA, PB, PC, LA, LB, LC, R, p, lo, hi, VmGradScalar{gd}, ox, oy, oz);
  grad_xyz[3 * m + 0] = ox;
  grad_xyz[3 * m + 1] = oy;
  grad_xyz[3 * m + 2] = oz;
}

template <bool PER_COMP>
static int vm_bwd_xyz(const TpPlanes& P, const VmLines& L, int R, const float* grad_out, const float* xyz, const float* mn,
                      const float* mx, int64_t M, float* grad_xyz, void* stream) {
  const int rc = vm_check(P, L, R, M, xyz, mn, mx, grad_out, grad_xyz);
  if (rc) return rc < 0 ? rc : 0;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (R % 4 == 0) && tp_planes_vec(P, 4) && vm_line_vec(L.a) && vm_line_vec(L.b) && vm_line_vec(L.c) &&
                   (!PER_COMP || (((uintptr_t)grad_out) & 15) == 0);
  const int blocks = dvgo_blocks(M, DVGO_BLOCK);
  if (vec)
    vm_bwd_xyz_kernel<4, PER_COMP><<<blocks, DVGO_BLOCK, 0, st>>>(P.a, P.b, P.c, L.a, L.b, L.c, R, grad_out, xyz, mn, mx, M, grad_xyz);
  else
    vm_bwd_xyz_kernel<1, PER_COMP><<<blocks, DVGO_BLOCK, 0, st>>>(P.a, P.b, P.c, L.a, L.b, L.c, R, grad_out, xyz, mn, mx, M, grad_xyz);
  DVGO_LAUNCH_CHECK();
  return 0;
}

extern "C" {

int dvgo_vm_bwd_xyz(const float* xy, int H_xy, int W_xy, int64_t sC_xy, int64_t sH_xy, int64_t sW_xy,
                    const float* yz, int H_yz, int W_yz, int64_t sC_yz, int64_t sH_yz, int64_t sW_yz,
                    const float* zx, int H_zx, int W_zx, int64_t sC_zx, int64_t sH_zx, int64_t sW_zx,
                    const float* l_xy, int N_xy, int64_t lC_xy, int64_t lN_xy,
                    const float* l_yz, int N_yz, int64_t lC_yz, int64_t lN_yz,
                    const float* l_zx, int N_zx, int64_t lC_zx, int64_t lN_zx,
                    int R, const float* grad_out, const float* xyz, const float* xyz_min, const float* xyz_max, int64_t M,
                    float* grad_xyz, void* stream) {
  return vm_bwd_xyz<true>(TP_PLANES(xy, yz, zx), VM_LINES(), R, grad_out, xyz, xyz_min, xyz_max, M, grad_xyz, stream);
}

int dvgo_vm_density_bwd_xyz(const float* xy, int H_xy, int W_xy, int64_t sC_xy, int64_t sH_xy, int64_t sW_xy,
                            const float* yz, int H_yz, int W_yz, int64_t sC_yz, int64_t sH_yz, int64_t sW_yz,
                            const float* zx, int H_zx, int W_zx, int64_t sC_zx, int64_t sH_zx, int64_t sW_zx,
                            const float* l_xy, int N_xy, int64_t lC_xy, int64_t lN_xy,
                            const float* l_yz, int N_yz, int64_t lC_yz, int64_t lN_yz,
                            const float* l_zx, int N_zx, int64_t lC_zx, int64_t lN_zx,
                            int R, const float* grad_out, const float* xyz, const float* xyz_min, const float* xyz_max,
                            int64_t M, float* grad_xyz, void* stream) {
  return vm_bwd_xyz<false>(TP_PLANES(xy, yz, zx), VM_LINES(), R, grad_out, xyz, xyz_min, xyz_max, M, grad_xyz, stream);
}

}  // extern "C"
