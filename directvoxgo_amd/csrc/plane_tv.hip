// Total-variation and L1 regularisers of plane-shaped parameters ([1,C,H,W] feature planes, [1,R,N,1] lines) added to
// their gradients: up to 8 tensors in ONE launch (include/dvgo_hip.h states the arithmetic).
// The 2-D counterpart of optim.hip's tv_rows_kernel, and shaped like it: a workgroup owns one contiguous row of one
// tensor, so the row's position (tensor, c, h) and the two h boundary tests are wave-uniform scalars, a thread does no
// integer division, and the five loads and the store of an element are contiguous across the wave.  The tensors of a
// tri-plane model are small (3 planes of 160^2 x 16 and 3 lines of 160 x 16 are 1.2 M floats): six launches of the
// 3-D kernel on [1,C,1,H,W] views cost more in launches than in traffic, and have no line form and no L1.
// Pure streaming: plain vector loads and stores, no LDS, no atomics; bitwise repeatable.
#include "common.h"

#define DVGO_PR_MAX 8

// Per tensor, a "row" is `R` elements `es` floats apart starting at c * sC + h * sH, and the column (w) neighbours of
// row element e are the row elements e -+ cs:
//   channels-last  (sC == 1, sW == C, sH == W*C): rows = H,     R = W*C, es = 1,  cs = C   (c runs inside the row)
//   channel-first  (sW == 1, sH == W, sC == H*W): rows = C * H, R = W,   es = 1,  cs = 1
//   any other dense layout                      : rows = C * H, R = W,   es = sW, cs = 1   (strided fallback)
struct PlaneRegTable {
  const float* p[DVGO_PR_MAX];
  float* g[DVGO_PR_MAX];
  int64_t sC[DVGO_PR_MAX], sH[DVGO_PR_MAX], es[DVGO_PR_MAX];
  int H[DVGO_PR_MAX], R[DVGO_PR_MAX], cs[DVGO_PR_MAX];
  float wh[DVGO_PR_MAX], ww[DVGO_PR_MAX], wl1[DVGO_PR_MAX];
  int start[DVGO_PR_MAX + 1];          // first workgroup of tensor k; start[n] = the grid size
  int n;
};

__device__ __forceinline__ float pr_clamp1(float v) { return fminf(fmaxf(v, -1.f), 1.f); }

template <bool DENSE>
__global__ void __launch_bounds__(DVGO_BLOCK)
plane_reg_rows_kernel(PlaneRegTable T) {
  const int b = blockIdx.x;
  int k = 0;
  while (k + 1 < T.n && b >= T.start[k + 1]) ++k;              // wave-uniform: at most 7 scalar compares
  const int row = b - T.start[k];
  const int H = T.H[k], R = T.R[k], cs = T.cs[k];
  const int c = row / H, h = row - c * H;                      // (channels-last: rows == H, c == 0)
  const int64_t sH = T.sH[k], es = T.es[k];
  const float ww = T.ww[k], wl1 = T.wl1[k];
  const float whm = (h == 0) ? 0.f : T.wh[k], whp = (h == H - 1) ? 0.f : T.wh[k];
  const int64_t ohm = (h == 0) ? 0 : -sH, ohp = (h == H - 1) ? 0 : sH;   // clamped: the loads stay in bounds
  const int64_t base = c * T.sC[k] + h * sH;
  const float* pr = T.p[k] + base;
  float* gr = T.g[k] + base;
  for (int e = threadIdx.x; e < R; e += blockDim.x) {
    const int64_t o = e * es;
    const float g0 = gr[o];
    if (!DENSE && g0 == 0.0f) continue;                        // (a -0.0 keeps its bits)
    const float p = pr[o];
    float g = 0.f;
    g += (e < cs      ? 0.f : ww * pr_clamp1(p - pr[o - cs * es]));
    g += (e >= R - cs ? 0.f : ww * pr_clamp1(p - pr[o + cs * es]));
    g += whm * pr_clamp1(p - pr[o + ohm]);
    g += whp * pr_clamp1(p - pr[o + ohp]);
    if (wl1 != 0.f) g += wl1 * (float)((p > 0.f) - (p < 0.f));
    gr[o] = g0 + g;
  }
}

extern "C" {

int dvgo_plane_reg_add_grad(const float* const* params, float* const* grads, const int64_t* sizes,
                            const int64_t* strides, const float* weights, int n_tensors, int dense_mode, void* stream) {
  if (n_tensors < 0 || n_tensors > DVGO_PR_MAX) return DVGO_EINVAL;
  if (n_tensors == 0) return 0;
  if (!params || !grads || !sizes || !strides || !weights) return DVGO_EINVAL;
  PlaneRegTable T;
  T.n = n_tensors;
  int64_t rows_total = 0;
  bool too_large = false;
  for (int k = 0; k < n_tensors; ++k) {
    int64_t C = sizes[3 * k], H = sizes[3 * k + 1], W = sizes[3 * k + 2];
    int64_t sC = strides[3 * k], sH = strides[3 * k + 1], sW = strides[3 * k + 2];
    float wh = weights[3 * k], ww = weights[3 * k + 1];
    if (C < 1 || H < 1 || W < 1 || !params[k] || !grads[k]) return DVGO_EINVAL;
    if (C >= ((int64_t)1 << 31) || H >= ((int64_t)1 << 31) || W >= ((int64_t)1 << 31) || !dvgo_fits(C * H) ||
        !dvgo_fits(C * H * W)) {
      too_large = true;                                        // (every tensor's arguments are judged first)
      continue;
    }
    // a column of nodes (W == 1, a line [1,R,N,1]) is the same stencil as a row of them: its two h terms become the two
    // w terms, in the same order and with the same weight, and the row then runs along memory
    if (W == 1 && H > 1) { W = H; H = 1; sW = sH; ww = wh; }
    const bool cl = (C == 1 || sC == 1) && (W == 1 || sW == C) && (H == 1 || sH == W * C);
    const bool cf = (W == 1 || sW == 1) && (H == 1 || sH == W) && (C == 1 || sC == H * W);
    T.p[k] = params[k]; T.g[k] = grads[k];
    T.sC[k] = sC; T.sH[k] = sH;
    T.H[k] = (int)H;
    T.R[k] = cl ? (int)(W * C) : (int)W;
    T.cs[k] = cl ? (int)C : 1;
    T.es[k] = (cl || cf) ? 1 : sW;
    T.wh[k] = wh; T.ww[k] = ww; T.wl1[k] = weights[3 * k + 2];
    T.start[k] = (int)rows_total;
    rows_total += cl ? H : C * H;
    if (!dvgo_fits(rows_total)) too_large = true;
  }
  if (too_large) return DVGO_ERANGE;
  for (int k = n_tensors; k <= DVGO_PR_MAX; ++k) T.start[k] = (int)rows_total;
  for (int k = n_tensors; k < DVGO_PR_MAX; ++k) {              // unused slots: defined values, never read
    T.p[k] = nullptr; T.g[k] = nullptr; T.sC[k] = T.sH[k] = T.es[k] = 0; T.H[k] = T.R[k] = T.cs[k] = 0;
    T.wh[k] = T.ww[k] = T.wl1[k] = 0.f;
  }
  hipStream_t s = (hipStream_t)stream;
  if (dense_mode)
    plane_reg_rows_kernel<true><<<(int)rows_total, DVGO_BLOCK, 0, s>>>(T);
  else
    plane_reg_rows_kernel<false><<<(int)rows_total, DVGO_BLOCK, 0, s>>>(T);
  DVGO_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
