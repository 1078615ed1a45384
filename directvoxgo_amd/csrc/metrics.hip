// Image metrics of rendered views against ground truth: SSIM (lib/utils.py:88-134, rgb_ssim) and the squared-error sum
// behind PSNR (run.py:116-117), for a batch of same-sized [H, W, 3] fp32 image pairs.
//
// Two launches per batch, whatever n is:
//   metrics_tile_kernel    one workgroup per (image, output tile of MT_H x MT_W): both images' tile + (fs-1) halo staged
//                          in LDS (all three channels, one coalesced pass over the interleaved rows); per channel the five
//                          blur inputs x, y, x^2, y^2, xy are blurred vertically into an fp64 LDS buffer, then horizontally,
//                          and the SSIM map is formed and summed.  The squared error of the pixels the tile owns is summed
//                          in the same pass over the staged pixels.  One (ssim, sse) partial per (image, tile).
//   metrics_reduce_kernel  one workgroup per image sums that image's partials in a fixed order.
// No atomics; an image's results depend only on its pixels and (H, W, fs), not on n or its place in the batch.
//
// Precision: the products x^2, y^2, xy are rounded to fp32, as the reference forms them on float32 arrays; everything from
// the blur on is fp64, as scipy.signal.convolve2d upcasts against the float64 filter.  In fp32 the variance
// E[x^2] - mu^2 cancels against c2 = 9e-4 (map entries off by ~1e-3).
#include "common.h"

#define MT_W 64                              // output tile columns
#define MT_H 8                               // output tile rows
#define MT_FS_MAX 16                         // largest filter_size the static LDS tile holds
#define MT_SR (MT_H + MT_FS_MAX - 1)         // staged rows (capacity)
#define MT_SC (MT_W + MT_FS_MAX - 1)         // staged columns (capacity, also the row stride)
// LDS: 2 x 3 x 23 x 79 x 4 B (staged pixels) + 5 x 8 x 79 x 8 B (vertical blurs) = 68.9 KB: two workgroups per CU

struct MetricsTaps {
  double f[MT_FS_MAX];
};

__device__ __forceinline__ double metrics_block_sum(double v, double* red) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();                           // red[] may still be read by a previous call
  if (lane == 0) red[w] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ void __launch_bounds__(256)
metrics_tile_kernel(const float* __restrict__ img0, const float* __restrict__ img1, int H, int W, int fs,
                    int tiles_x, int tiles_per_image, MetricsTaps taps, double c1, double c2,
                    double* __restrict__ partials, float* __restrict__ ssim_map) {
  __shared__ float sx[3][MT_SR][MT_SC];
  __shared__ float sy[3][MT_SR][MT_SC];
  __shared__ double vb[5][MT_H][MT_SC];
  __shared__ double f[MT_FS_MAX];
  __shared__ double red[4];

  const int tid = threadIdx.x;
  const int img = blockIdx.x / tiles_per_image;
  const int t = blockIdx.x - img * tiles_per_image;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int Ho = H - fs + 1, Wo = W - fs + 1;
  const int r0 = ty * MT_H, c0 = tx * MT_W;
  const int nor = min(MT_H, Ho - r0), noc = min(MT_W, Wo - c0);       // output rows / columns of this tile
  const int nrs = nor + fs - 1, ncs = noc + fs - 1;                    // staged rows / columns
  // pixels whose squared error this tile counts: its own MT_H x MT_W block, up to the image edge for the last tile
  const int own_r = (ty == (Ho - 1) / MT_H) ? H - r0 : MT_H;
  const int own_c = (tx == tiles_x - 1) ? W - c0 : MT_W;

  if (tid < fs) f[tid] = taps.f[tid];
  const int64_t base = (int64_t)img * H * W * 3;
  const float* __restrict__ a = img0 + base;
  const float* __restrict__ b = img1 + base;
  double sse = 0.0;
  const int row_len = ncs * 3;
  for (int it = tid; it < nrs * row_len; it += 256) {
    const int rr = it / row_len, e = it - rr * row_len;
    const int cc = e / 3, ch = e - cc * 3;
    const int g = ((r0 + rr) * W + c0) * 3 + e;
    const float x = a[g], y = b[g];
    sx[ch][rr][cc] = x;
    sy[ch][rr][cc] = y;
    if (rr < own_r && cc < own_c) {
      const float d = x - y;                 // run.py:117 np.square(rgb - gt) on float32
      sse += (double)(d * d);
    }
  }
  __syncthreads();

  double ssum = 0.0;
  for (int ch = 0; ch < 3; ++ch) {
    // vertical blur of the five inputs: rows [0, nor), staged columns [0, ncs)
    for (int it = tid; it < nor * ncs; it += 256) {
      const int r = it / ncs, c = it - r * ncs;
      double m0 = 0.0, m1 = 0.0, m00 = 0.0, m11 = 0.0, m01 = 0.0;
      for (int k = 0; k < fs; ++k) {
        const float x = sx[ch][r + k][c], y = sy[ch][r + k][c];
        const double w = f[k];
        m0 += w * (double)x;
        m1 += w * (double)y;
        m00 += w * (double)(x * x);
        m11 += w * (double)(y * y);
        m01 += w * (double)(x * y);
      }
      vb[0][r][c] = m0; vb[1][r][c] = m1; vb[2][r][c] = m00; vb[3][r][c] = m11; vb[4][r][c] = m01;
    }
    __syncthreads();
    // horizontal blur and the map (lib/utils.py:112-133)
    for (int it = tid; it < nor * noc; it += 256) {
      const int r = it / noc, c = it - r * noc;
      double mu0 = 0.0, mu1 = 0.0, e00 = 0.0, e11 = 0.0, e01 = 0.0;
      for (int k = 0; k < fs; ++k) {
        const double w = f[k];
        mu0 += w * vb[0][r][c + k];
        mu1 += w * vb[1][r][c + k];
        e00 += w * vb[2][r][c + k];
        e11 += w * vb[3][r][c + k];
        e01 += w * vb[4][r][c + k];
      }
      const double mu00 = mu0 * mu0, mu11 = mu1 * mu1, mu01 = mu0 * mu1;
      const double s00 = fmax(0.0, e00 - mu00);
      const double s11 = fmax(0.0, e11 - mu11);
      double s01 = e01 - mu01;
      const double lim = sqrt(s00 * s11);
      s01 = s01 > 0.0 ? fmin(lim, s01) : (s01 < 0.0 ? -fmin(lim, -s01) : s01 * 0.0);   // sign(s01) * min(lim, |s01|)
      const double numer = (2.0 * mu01 + c1) * (2.0 * s01 + c2);
      const double denom = (mu00 + mu11 + c1) * (s00 + s11 + c2);
      const double v = numer / denom;
      ssum += v;
      if (ssim_map)
        ssim_map[((int64_t)img * Ho * Wo + (int64_t)(r0 + r) * Wo + (c0 + c)) * 3 + ch] = (float)v;
    }
    __syncthreads();
  }

  const double ts = metrics_block_sum(ssum, red);
  const double te = metrics_block_sum(sse, red);
  if (tid == 0) {
    partials[2 * (int64_t)blockIdx.x] = ts;
    partials[2 * (int64_t)blockIdx.x + 1] = te;
  }
}

// one workgroup per image: its tiles' partials in a fixed order (strided per thread, then the block sum)
__global__ void __launch_bounds__(256)
metrics_reduce_kernel(const double* __restrict__ partials, int tiles_per_image, double* __restrict__ ssim_sum,
                      double* __restrict__ sse) {
  __shared__ double red[4];
  const double* p = partials + 2 * (int64_t)blockIdx.x * tiles_per_image;
  double s = 0.0, e = 0.0;
  for (int t = threadIdx.x; t < tiles_per_image; t += 256) {
    s += p[2 * t];
    e += p[2 * t + 1];
  }
  s = metrics_block_sum(s, red);
  e = metrics_block_sum(e, red);
  if (threadIdx.x == 0) {
    ssim_sum[blockIdx.x] = s;
    sse[blockIdx.x] = e;
  }
}

static int64_t metrics_tiles(int H, int W, int fs) {
  return (int64_t)((H - fs + 1 + MT_H - 1) / MT_H) * ((W - fs + 1 + MT_W - 1) / MT_W);
}

// sizes shared by both entry points: DVGO_EINVAL / DVGO_ERANGE, or 0
static int metrics_check_sizes(int64_t n, int H, int W, int fs) {
  if (n < 0 || H <= 0 || W <= 0 || fs < 1) return DVGO_EINVAL;
  if (H < fs || W < fs) return DVGO_EINVAL;          // the reference's map would be empty (np.mean -> nan)
  if (fs > MT_FS_MAX) return DVGO_ERANGE;
  if ((int64_t)H * W * 3 >= ((int64_t)1 << 31)) return DVGO_ERANGE;
  if (n * metrics_tiles(H, W, fs) >= ((int64_t)1 << 31)) return DVGO_ERANGE;
  return 0;
}

int64_t dvgo_image_metrics_workspace_bytes(int64_t n, int H, int W, int filter_size) {
  const int rc = metrics_check_sizes(n, H, W, filter_size);
  if (rc) return rc;
  return n * metrics_tiles(H, W, filter_size) * 2 * (int64_t)sizeof(double);
}

int dvgo_image_metrics(const float* img0, const float* img1, int64_t n, int H, int W, const double* taps,
                       int filter_size, double c1, double c2, double* ssim_sum, double* sse, float* ssim_map,
                       void* workspace, int64_t workspace_bytes, void* stream) {
  if (n < 0) return DVGO_EINVAL;
  if (n == 0) return 0;
  const int rc = metrics_check_sizes(n, H, W, filter_size);
  if (rc) return rc;
  if (!img0 || !img1 || !taps || !ssim_sum || !sse || !workspace) return DVGO_EINVAL;
  if (workspace_bytes < dvgo_image_metrics_workspace_bytes(n, H, W, filter_size)) return DVGO_EINVAL;
  MetricsTaps t = {};
  for (int k = 0; k < filter_size; ++k) t.f[k] = taps[k];
  const int tiles_x = (W - filter_size + 1 + MT_W - 1) / MT_W;
  const int tiles = (int)metrics_tiles(H, W, filter_size);
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)workspace;
  metrics_tile_kernel<<<(int)(n * tiles), 256, 0, s>>>(img0, img1, H, W, filter_size, tiles_x, tiles, t, c1, c2, part,
                                                       ssim_map);
  DVGO_LAUNCH_CHECK();
  metrics_reduce_kernel<<<(int)n, 256, 0, s>>>(part, tiles, ssim_sum, sse);
  DVGO_LAUNCH_CHECK();
  return 0;
}
