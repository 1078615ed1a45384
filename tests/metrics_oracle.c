/*
 * metrics_oracle.c -- CPU statement of the image metrics (TEST INFRASTRUCTURE ONLY; tests/metrics_oracle.py builds and
 * loads it).  Independent of scipy so that GPU tests can check 800x800 views.
 *
 *   lib/utils.py:88-134  rgb_ssim: separable 'valid' Gaussian blur per channel of x, y, x^2, y^2, xy; the products are
 *                        float32 (numpy on float32 images), everything from the blur on is float64 (convolve2d upcasts
 *                        against the float64 filter); variance clip, covariance sign clip, map, mean over all entries.
 *   run.py:117           PSNR = -10 log10(mean((rgb - gt)^2)) with the difference and its square in float32; the sum
 *                        here is float64.
 * The filter is symmetric, so convolve2d's flip changes nothing: out[i] = sum_k f[k] in[i + k].
 * Compile with -ffp-contract=off.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

/* a, b [H,W,3]; f [fs] float64 taps.  -> *ssim_sum (sum over the map), *sse; map [H-fs+1, W-fs+1, 3] when not NULL. */
int ora_image_metrics(const float* a, const float* b, int H, int W, const double* f, int fs, double c1, double c2,
                      double* map, double* ssim_sum, double* sse) {
  if (H < fs || W < fs || fs < 1) return -1;
  const int Ho = H - fs + 1, Wo = W - fs + 1;
  double* in = malloc(sizeof(double) * 5 * (size_t)H * W);
  double* v = malloc(sizeof(double) * 5 * (size_t)Ho * W);
  if (!in || !v) { free(in); free(v); return -2; }
  double e = 0.0;
  for (int64_t i = 0; i < (int64_t)H * W * 3; ++i) {
    const float d = a[i] - b[i];
    const float d2 = d * d;
    e += (double)d2;
  }
  double s = 0.0;
  for (int ch = 0; ch < 3; ++ch) {
    for (int64_t p = 0; p < (int64_t)H * W; ++p) {
      const float x = a[p * 3 + ch], y = b[p * 3 + ch];
      const float xx = x * x, yy = y * y, xy = x * y;
      in[0 * (int64_t)H * W + p] = (double)x;
      in[1 * (int64_t)H * W + p] = (double)y;
      in[2 * (int64_t)H * W + p] = (double)xx;
      in[3 * (int64_t)H * W + p] = (double)yy;
      in[4 * (int64_t)H * W + p] = (double)xy;
    }
    for (int q = 0; q < 5; ++q)
      for (int r = 0; r < Ho; ++r)
        for (int c = 0; c < W; ++c) {
          double acc = 0.0;
          for (int k = 0; k < fs; ++k) acc += f[k] * in[(int64_t)q * H * W + (int64_t)(r + k) * W + c];
          v[(int64_t)q * Ho * W + (int64_t)r * W + c] = acc;
        }
    for (int r = 0; r < Ho; ++r)
      for (int c = 0; c < Wo; ++c) {
        double m[5];
        for (int q = 0; q < 5; ++q) {
          double acc = 0.0;
          for (int k = 0; k < fs; ++k) acc += f[k] * v[(int64_t)q * Ho * W + (int64_t)r * W + c + k];
          m[q] = acc;
        }
        const double mu00 = m[0] * m[0], mu11 = m[1] * m[1], mu01 = m[0] * m[1];
        double s00 = m[2] - mu00, s11 = m[3] - mu11, s01 = m[4] - mu01;
        s00 = s00 > 0.0 ? s00 : 0.0;                                   /* np.maximum(0., .) */
        s11 = s11 > 0.0 ? s11 : 0.0;
        const double lim = sqrt(s00 * s11);
        const double mag = fabs(s01) < lim ? fabs(s01) : lim;         /* np.minimum(sqrt(.), abs(.)) */
        s01 = (s01 > 0.0) ? mag : (s01 < 0.0 ? -mag : 0.0);          /* np.sign(.) * ... */
        const double val = ((2.0 * mu01 + c1) * (2.0 * s01 + c2)) / ((mu00 + mu11 + c1) * (s00 + s11 + c2));
        if (map) map[((int64_t)r * Wo + c) * 3 + ch] = val;
        s += val;
      }
  }
  free(in);
  free(v);
  *ssim_sum = s;
  *sse = e;
  return 0;
}
