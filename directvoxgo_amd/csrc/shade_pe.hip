// Positional-encoding colour head for gfx950: the `posbase_pe > 0` branch of the reference's fine-stage model
// (lib/dvgo.py:528-534 of the reference):
//   pos_emb = cat([pts, sin(pts (x) posfreq), cos(pts (x) posfreq)])          [M, 3 + 6P]
//   rgb     = sigmoid(rgbnet(cat([pos_emb, viewdirs_emb[ray_id]])))           no diffuse term, k0 unused
// with rgbnet = Linear(d_in, 128) + ReLU, Linear(128, 128) + ReLU, Linear(128, 3), d_in = 3 + 6P + 3 + 6V <= 96.
//
// The layer-1 input row is never written to memory: every kernel that needs it rebuilds it from the sample position
// (12 B) and the per-ray view embedding.  sin / cos are sinf / cosf on the fp32 argument x * 2^j (the scaling is
// exact), as dvgo_viewdir_embed computes the view embedding; the fast hardware sine would lose accuracy at the
// arguments P = 10 reaches (2^9 |x| ~ 770 rad).
//
// The matrix work uses the layout of csrc/shade.hip (see its header): every layer computed transposed on
// v_mfma_f32_32x32x2_f32 (an exact fp32 FMA chain), weights as the A operand pre-permuted in LDS, activations as the B
// operand straight from the previous layer's accumulator registers.  Layer 1 runs k-step by k-step: the two input
// features a lane contributes to a step are computed right before that step's four MFMAs, so no input row is held.
//
// Kernels:
//   pe_positions_kernel  pts = start + dir * dist of the fused march's kept samples (dvgo_march_positions)
//   pe_fwd_kernel        rgb; training: H1, H2 [M,128] and the ReLU sign bits (32 B / sample)
//   pe_bwd_kernel        gz = g_rgb * sigmoid', G1 = relu'(H1) (W2^T (relu'(H2) (W3^T gz)))   (no input gradient)
//   pe_wgrad_kernel      per-workgroup partial dW1 = G1^T X (X rebuilt), dW2 = G2^T H1, dW3 = gz^T H2, biases
//   pe_reduce_kernel     sum of the partials into the compact record of include/dvgo_hip.h
#include "common.h"
#include "x3.h"     // f32x16

#define PE_WIDTH 128
#define PE_T (PE_WIDTH / 32)
#define PE_MAX_DIN 96
#define PE_MAX_S1 (PE_MAX_DIN / 2)
#define PE_MAX_FREQ 16
#define PE_THREADS 512          // forward / data gradients: 8 wavefronts (two per SIMD), one workgroup per CU (LDS)
#define PE_WAVES (PE_THREADS / 64)
#define PE_WG_THREADS 256       // weight gradients: wave w owns out-feature tile w
#define PE_STAGE_STRIDE 36
#define PE_ROW_STRIDE (PE_WIDTH + 32)   // LDS row stride of the weight-gradient tiles: the two rows of a k-step sit in
                                        // opposite bank halves
#define PE_X_STRIDE (PE_MAX_DIN + 32)

__device__ __forceinline__ int pe_acc_feature(int t, int r, int h) { return 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h; }

// What input feature k of layer 1 is, as one int: bits 0-2 kind (0 position, 1 sin, 2 cos, 3 view embedding,
// 4 zero padding), bits 3-4 axis, bits 5+ frequency index (kinds 1, 2) or embedding column (kind 3).
__device__ __forceinline__ int pe_kinfo(int k, int P, int d_in) {
  const int npos = 3 + 6 * P;
  if (k < 3) return 0 | (k << 3);
  if (k < npos) {
    int i = k - 3;
    const int kind = i < 3 * P ? 1 : 2;
    if (kind == 2) i -= 3 * P;
    const int a = i / P, j = i - a * P;      // flatten order of (pts.unsqueeze(-1) * posfreq).flatten(-2)
    return kind | (a << 3) | (j << 5);
  }
  if (k < d_in) return 3 | ((k - npos) << 5);
  return 4;
}

__device__ __forceinline__ float pe_feature(int info, float px, float py, float pz, const float* __restrict__ freq,
                                            const float* __restrict__ er) {
  const int kind = info & 7, a = (info >> 3) & 3, j = info >> 5;
  if (kind == 3) return er[j];
  if (kind == 4) return 0.0f;
  const float xa = a == 0 ? px : (a == 1 ? py : pz);
  if (kind == 0) return xa;
  const float arg = xa * freq[j];
  float s, c;
  sincosf(arg, &s, &c);
  return kind == 1 ? s : c;
}

// Row-major store of one 32(sample) x 32(feature) accumulator tile through a wave-private LDS patch (8 full 128-B
// row segments per wave instruction instead of 32 rows x 32 B).  Same wave writes and reads: no barrier.
__device__ __forceinline__ void pe_store_tile(float* __restrict__ stage, const f32x16& acc, float* __restrict__ dst,
                                              int row_stride, int lane, int rows_valid) {
  const int smp = lane & 31, h = lane >> 5;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    *reinterpret_cast<float4*>(stage + smp * PE_STAGE_STRIDE + 8 * q + 4 * h) =
        make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
  const int c = lane & 7;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = (lane >> 3) + 8 * i;
    const float4 v = *reinterpret_cast<const float4*>(stage + r * PE_STAGE_STRIDE + 4 * c);
    if (r < rows_valid) *reinterpret_cast<float4*>(dst + (int64_t)r * row_stride + 4 * c) = v;
  }
}

// ----------------------------------------------------------------------------------
// Sample positions of the fused march's kept samples: the expression of march_gather / dvgo_sample_pos
// (render_utils_kernel.cu:178-181, contracted), so pts equal sample_pts_on_rays' ray_pts bit for bit.
// ----------------------------------------------------------------------------------
__global__ void __launch_bounds__(DVGO_BLOCK)
pe_positions_kernel(const float* __restrict__ start, const float* __restrict__ dirs, const int64_t* __restrict__ ray_id,
                    const int64_t* __restrict__ step_id, int64_t M, float stepdist, float* __restrict__ pts) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  float px, py, pz;
  march_pos(start, dirs, ray_id[i], stepdist, (int)step_id[i], px, py, pz);
  pts[3 * i + 0] = px;
  pts[3 * i + 1] = py;
  pts[3 * i + 2] = pz;
}

// ----------------------------------------------------------------------------------
// Forward
// ----------------------------------------------------------------------------------
struct PeFwdLds {
  float w1a[PE_T][PE_MAX_S1][64];      // [out tile][k-step][lane]: W1[32t + (lane&31)][2s + (lane>>5)]
  float w2a[PE_T][PE_T][16][64];       // [out tile][in tile][reg][lane]
  float w3p[3][2][PE_T * 16];          // [c][lane half][in tile*16 + reg]
  float b1p[2][PE_T * 16];
  float b2p[2][PE_T * 16];
  float b3[4];
  float freq[PE_MAX_FREQ];
  int kinfo[PE_MAX_DIN];
};

__global__ void __launch_bounds__(PE_THREADS)
pe_fwd_kernel(const float* __restrict__ pts, const float* __restrict__ freq, int P, const float* __restrict__ emb, int E,
              const int64_t* __restrict__ ray_id, int64_t M, const float* __restrict__ W1, const float* __restrict__ b1,
              const float* __restrict__ W2, const float* __restrict__ b2, const float* __restrict__ W3,
              const float* __restrict__ b3, int d_in, float* __restrict__ rgb, float* __restrict__ H1, float* __restrict__ H2,
              unsigned long long* __restrict__ masks) {
  __shared__ PeFwdLds L;
  __shared__ __attribute__((aligned(16))) float s_stage[PE_WAVES][32 * PE_STAGE_STRIDE];
  const int S1 = (d_in + 1) / 2;
  {
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int i = tid; i < PE_T * PE_MAX_S1 * 64; i += nt) {
      const int l = i & 63, s = (i >> 6) % PE_MAX_S1, t = (i >> 6) / PE_MAX_S1;
      const int k = 2 * s + (l >> 5);
      (&L.w1a[0][0][0])[i] = (k < d_in) ? W1[(32 * t + (l & 31)) * d_in + k] : 0.0f;
    }
    for (int i = tid; i < PE_T * PE_T * 16 * 64; i += nt) {
      const int l = i & 63, r = (i >> 6) & 15, t = (i >> 10) % PE_T, t2 = (i >> 10) / PE_T;
      (&L.w2a[0][0][0][0])[i] = W2[(32 * t2 + (l & 31)) * PE_WIDTH + pe_acc_feature(t, r, l >> 5)];
    }
    for (int i = tid; i < 3 * 2 * PE_T * 16; i += nt) {
      const int tr = i % (PE_T * 16), h = (i / (PE_T * 16)) & 1, c = i / (2 * PE_T * 16);
      (&L.w3p[0][0][0])[i] = W3[c * PE_WIDTH + pe_acc_feature(tr >> 4, tr & 15, h)];
    }
    for (int i = tid; i < 2 * PE_T * 16; i += nt) {
      const int tr = i % (PE_T * 16), h = i / (PE_T * 16);
      const int f = pe_acc_feature(tr >> 4, tr & 15, h);
      (&L.b1p[0][0])[i] = b1[f];
      (&L.b2p[0][0])[i] = b2[f];
    }
    if (tid < 3) L.b3[tid] = b3[tid];
    if (tid < PE_MAX_FREQ) L.freq[tid] = tid < P ? freq[tid] : 0.0f;
    if (tid < PE_MAX_DIN) L.kinfo[tid] = pe_kinfo(tid, P, d_in);
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, h = lane >> 5;
  float* stage = s_stage[threadIdx.x >> 6];
  const int64_t n_tiles = (M + 31) / 32;
  const int64_t gw = (int64_t)blockIdx.x * PE_WAVES + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * PE_WAVES;
  for (int64_t tile = gw; tile < n_tiles; tile += nw) {
    const int64_t row = tile * 32 + (lane & 31);
    const bool valid = row < M;
    const int64_t rowc = valid ? row : (M - 1);
    const int rows_valid = (int)(M - tile * 32 < 32 ? M - tile * 32 : 32);
    const float px = pts[3 * rowc], py = pts[3 * rowc + 1], pz = pts[3 * rowc + 2];
    const float* er = emb + ray_id[rowc] * E;
    f32x16 acc1[PE_T];
#pragma unroll
    for (int t = 0; t < PE_T; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc1[t][r] = L.b1p[h][t * 16 + r];
    // layer 1, one k-step at a time: this lane's input feature k = 2s + h of its row, then the step's four MFMAs
#pragma unroll 1
    for (int s = 0; s < S1; ++s) {
      const float x = pe_feature(L.kinfo[2 * s + h], px, py, pz, L.freq, er);
#pragma unroll
      for (int t = 0; t < PE_T; ++t) acc1[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(L.w1a[t][s][lane], x, acc1[t], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < PE_T; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc1[t][r] = dvgo_relu(acc1[t][r]);
    // layer 2 one 32-feature output tile at a time, each consumed at once by layer 3 (and the H2 store)
    float p[3] = {0.0f, 0.0f, 0.0f};
    unsigned long long mask2 = 0ull;
#pragma unroll 1
    for (int t2 = 0; t2 < PE_T; ++t2) {
      f32x16 acc2;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc2[r] = L.b2p[h][t2 * 16 + r];
#pragma unroll
      for (int t = 0; t < PE_T; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(L.w2a[t2][t][r][lane], acc1[t][r], acc2, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) acc2[r] = dvgo_relu(acc2[r]);
      if (H1 != nullptr) {
        unsigned int bits = 0u;
#pragma unroll
        for (int r = 0; r < 16; ++r) bits |= dvgo_relu_bit(acc2[r]) << r;
        mask2 |= (unsigned long long)bits << (16 * t2);
        pe_store_tile(stage, acc2, H2 + tile * 32 * PE_WIDTH + 32 * t2, PE_WIDTH, lane, rows_valid);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int r = 0; r < 16; ++r) p[c] = fmaf(L.w3p[c][h][t2 * 16 + r], acc2[r], p[c]);
      }
    }
    float z[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) z[c] = p[c] + __shfl_xor(p[c], 32) + L.b3[c];
    if (valid) {
      if (h == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[row * 3 + c] = 1.0f / (1.0f + expf(-z[c]));
      }
      if (H1 != nullptr) {
        unsigned long long mask1 = 0ull;
#pragma unroll
        for (int t = 0; t < PE_T; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) mask1 |= (unsigned long long)dvgo_relu_bit(acc1[t][r]) << (16 * t + r);
        masks[(row * 2 + 0) * 2 + h] = mask1;
        masks[(row * 2 + 1) * 2 + h] = mask2;
      }
    }
    if (H1 != nullptr) {
#pragma unroll
      for (int t = 0; t < PE_T; ++t) pe_store_tile(stage, acc1[t], H1 + tile * 32 * PE_WIDTH + 32 * t, PE_WIDTH, lane, rows_valid);
    }
  }
}

// ----------------------------------------------------------------------------------
// Backward, data path.  Per 32-row tile:
//   gz = g_rgb * rgb * (1 - rgb)
//   G2 = (H2 > 0) * (W3^T gz)        VALU, accumulator layout (not stored: pe_wgrad_kernel rebuilds it, same bits)
//   G1 = (H1 > 0) * (W2^T G2)        MFMA, A = W2^T pre-permuted so that G2's registers are the B operands
// Positions and view directions carry no gradient, so there is no W1^T G1.
// ----------------------------------------------------------------------------------
struct PeBwdLds {
  float w2ta[PE_T][PE_T][16][64];      // [in tile][out tile][reg][lane] = W2[f_out(t2,r,lane>>5)][32*t_in + (lane&31)]
  float w3p[3][2][PE_T * 16];
};

__global__ void __launch_bounds__(PE_THREADS)
pe_bwd_kernel(const float* __restrict__ g_rgb, const float* __restrict__ rgb, const unsigned long long* __restrict__ masks,
              int64_t M, const float* __restrict__ W2, const float* __restrict__ W3, float* __restrict__ G1,
              float* __restrict__ gz_out) {
  __shared__ PeBwdLds L;
  __shared__ __attribute__((aligned(16))) float s_stage[PE_WAVES][32 * PE_STAGE_STRIDE];
  {
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int i = tid; i < PE_T * PE_T * 16 * 64; i += nt) {
      const int l = i & 63, r = (i >> 6) & 15, t2 = (i >> 10) % PE_T, tin = (i >> 10) / PE_T;
      (&L.w2ta[0][0][0][0])[i] = W2[pe_acc_feature(t2, r, l >> 5) * PE_WIDTH + 32 * tin + (l & 31)];
    }
    for (int i = tid; i < 3 * 2 * PE_T * 16; i += nt) {
      const int tr = i % (PE_T * 16), h = (i / (PE_T * 16)) & 1, c = i / (2 * PE_T * 16);
      (&L.w3p[0][0][0])[i] = W3[c * PE_WIDTH + pe_acc_feature(tr >> 4, tr & 15, h)];
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, h = lane >> 5;
  float* stage = s_stage[threadIdx.x >> 6];
  const int64_t n_tiles = (M + 31) / 32;
  const int64_t gw = (int64_t)blockIdx.x * PE_WAVES + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * PE_WAVES;
  for (int64_t tile = gw; tile < n_tiles; tile += nw) {
    const int64_t row = tile * 32 + (lane & 31);
    const bool valid = row < M;
    const int64_t rowc = valid ? row : (M - 1);
    float gz[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float o = rgb[rowc * 3 + c];
      gz[c] = valid ? g_rgb[rowc * 3 + c] * o * (1.0f - o) : 0.0f;
    }
    if (valid && h == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) gz_out[row * 3 + c] = gz[c];
    }
    const unsigned long long m1 = masks[(rowc * 2 + 0) * 2 + h];
    const unsigned long long m2 = masks[(rowc * 2 + 1) * 2 + h];
    f32x16 g2[PE_T];
#pragma unroll
    for (int t2 = 0; t2 < PE_T; ++t2) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v = fmaf(L.w3p[2][h][t2 * 16 + r], gz[2],
                             fmaf(L.w3p[1][h][t2 * 16 + r], gz[1], L.w3p[0][h][t2 * 16 + r] * gz[0]));
        g2[t2][r] = ((m2 >> (16 * t2 + r)) & 1ull) ? v : 0.0f;
      }
    }
    const int rows_valid = (int)(M - tile * 32 < 32 ? M - tile * 32 : 32);
#pragma unroll 1
    for (int tin = 0; tin < PE_T; ++tin) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
      for (int t2 = 0; t2 < PE_T; ++t2) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(L.w2ta[tin][t2][r][lane], g2[t2][r], acc, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = ((m1 >> (16 * tin + r)) & 1ull) ? acc[r] : 0.0f;
      pe_store_tile(stage, acc, G1 + tile * 32 * PE_WIDTH + 32 * tin, PE_WIDTH, lane, rows_valid);
    }
  }
}

// ----------------------------------------------------------------------------------
// Backward, weight gradients.  A contraction over rows of row-major [M, features] operands:
//   A[i = out feature][k = row]  lane (i, h) reads G[row 2s + h][f0 + i]
//   B[k = row][j = in feature]   lane (j, h) reads H[row 2s + h][f0' + j]
// The workgroup stages one 32-row tile of G1, H1, H2, gz, the layer-2 sign bits and the rebuilt layer-1 input X in
// LDS; wave w then owns out-feature tile w: dW2 (4 accumulator tiles), dW1 (up to 3 tiles: d_in <= 96), and on the
// VALU dW3 and the bias sums.  G2 is rebuilt from gz and the sign bits with the data-path kernel's expression.
// Two workgroups per CU (79 KB of LDS each): one computes while the other stages its next tile.
// Each workgroup writes its partial sums, already in the compact record's layout, to part[blockIdx].
// ----------------------------------------------------------------------------------
struct PeWgradLds {
  float g1[32][PE_ROW_STRIDE], h1[32][PE_ROW_STRIDE], h2[32][PE_ROW_STRIDE];
  float x[32][PE_X_STRIDE];
  float gz[32][4];
  unsigned long long m2[32][2];
  float freq[PE_MAX_FREQ];
  int kinfo[PE_MAX_DIN];
};

__global__ void __launch_bounds__(PE_WG_THREADS, 2)
pe_wgrad_kernel(const float* __restrict__ G1, const float* __restrict__ gz, const unsigned long long* __restrict__ masks,
                const float* __restrict__ W3, const float* __restrict__ H1, const float* __restrict__ H2,
                const float* __restrict__ pts, const float* __restrict__ freq, int P, const float* __restrict__ emb, int E,
                const int64_t* __restrict__ ray_id, int64_t M, int d_in, int rec_size, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) PeWgradLds L;
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, j = lane & 31, w = tid >> 6;
  if (tid < PE_MAX_FREQ) L.freq[tid] = tid < P ? freq[tid] : 0.0f;
  if (tid < PE_MAX_DIN) L.kinfo[tid] = pe_kinfo(tid, P, d_in);
  f32x16 aW2[PE_T], aW1[3];
#pragma unroll
  for (int t = 0; t < PE_T; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) aW2[t][r] = 0.0f;
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) aW1[t][r] = 0.0f;
  const int n_x_tiles = (d_in + 31) / 32;
  float vW3[3] = {0.0f, 0.0f, 0.0f}, sb1 = 0.0f, sb2 = 0.0f, sgz = 0.0f;
  // this lane's layer-2 feature f = 32w + j: its W3 column and the place of its sign bit in the forward's masks
  const int f = 32 * w + j;
  const float w30 = W3[f], w31 = W3[PE_WIDTH + f], w32 = W3[2 * PE_WIDTH + f];
  const int m_half = (j >> 2) & 1, m_bit = 16 * w + (j & 3) + 4 * (j >> 3);
  const int64_t n_tiles = (M + 31) / 32;
  __syncthreads();
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t r0 = tile * 32;
    // stage: G1 / H1 / H2 rows as float4 (rows past M as zeros)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = tid + PE_WG_THREADS * q;            // 1024 float4 per 32 x 128 tile
      const int rr = e >> 5, c4 = (e & 31) * 4;
      const int64_t row = r0 + rr;
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a, c = a;
      if (row < M) {
        a = *reinterpret_cast<const float4*>(G1 + row * PE_WIDTH + c4);
        b = *reinterpret_cast<const float4*>(H1 + row * PE_WIDTH + c4);
        c = *reinterpret_cast<const float4*>(H2 + row * PE_WIDTH + c4);
      }
      *reinterpret_cast<float4*>(&L.g1[rr][c4]) = a;
      *reinterpret_cast<float4*>(&L.h1[rr][c4]) = b;
      *reinterpret_cast<float4*>(&L.h2[rr][c4]) = c;
    }
    if (tid < 64) {
      const int rr = tid >> 1;
      const int64_t row = r0 + rr;
      L.m2[rr][tid & 1] = row < M ? masks[(row * 2 + 1) * 2 + (tid & 1)] : 0ull;
    } else if (tid < 64 + 32) {
      const int rr = tid - 64;
      const int64_t row = r0 + rr;
#pragma unroll
      for (int c = 0; c < 3; ++c) L.gz[rr][c] = row < M ? gz[row * 3 + c] : 0.0f;
      L.gz[rr][3] = 0.0f;
    }
    {   // X: 8 threads per row, columns c, c + 8, ... (rows past M as zeros)
      const int rr = tid >> 3, c0 = tid & 7;
      const int64_t row = r0 + rr;
      if (row < M) {
        const float px = pts[3 * row], py = pts[3 * row + 1], pz = pts[3 * row + 2];
        const float* er = emb + ray_id[row] * E;
        for (int k = c0; k < 32 * n_x_tiles; k += 8) L.x[rr][k] = pe_feature(L.kinfo[k], px, py, pz, L.freq, er);
      } else {
        for (int k = c0; k < 32 * n_x_tiles; k += 8) L.x[rr][k] = 0.0f;
      }
    }
    __syncthreads();
#pragma unroll 2
    for (int s = 0; s < 16; ++s) {
      const int row = 2 * s + h;
      const float g0 = L.gz[row][0], g1v = L.gz[row][1], g2v = L.gz[row][2];
      const float v = fmaf(w32, g2v, fmaf(w31, g1v, w30 * g0));
      const float a2 = ((L.m2[row][m_half] >> m_bit) & 1ull) ? v : 0.0f;
      const float a1 = L.g1[row][f];
      const float hh = L.h2[row][f];
      sb1 += a1;
      sb2 += a2;
      vW3[0] = fmaf(g0, hh, vW3[0]);
      vW3[1] = fmaf(g1v, hh, vW3[1]);
      vW3[2] = fmaf(g2v, hh, vW3[2]);
      if (j < 3) sgz += L.gz[row][j];
#pragma unroll
      for (int t = 0; t < PE_T; ++t) aW2[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2, L.h1[row][32 * t + j], aW2[t], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < 3; ++t)
        if (t < n_x_tiles) aW1[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, L.x[row][32 * t + j], aW1[t], 0, 0, 0);
    }
    __syncthreads();
  }
  // partial record { dW2 [W][W], dW1 [W][d_in], dW3 [3][W], db1 [W], db2 [W], db3 [3] }
  float* pr = part + (int64_t)blockIdx.x * rec_size;
  float* pW1 = pr + PE_WIDTH * PE_WIDTH;
  float* pW3 = pW1 + PE_WIDTH * d_in;
  float* pb1 = pW3 + 3 * PE_WIDTH;
  float* pb2 = pb1 + PE_WIDTH;
  float* pb3 = pb2 + PE_WIDTH;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = 32 * w + pe_acc_feature(0, r, h);
#pragma unroll
    for (int t = 0; t < PE_T; ++t) pr[i * PE_WIDTH + 32 * t + j] = aW2[t][r];
#pragma unroll
    for (int t = 0; t < 3; ++t)
      if (32 * t + j < d_in) pW1[i * d_in + 32 * t + j] = aW1[t][r];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) vW3[c] += __shfl_xor(vW3[c], 32);
  sb1 += __shfl_xor(sb1, 32);
  sb2 += __shfl_xor(sb2, 32);
  sgz += __shfl_xor(sgz, 32);
  if (h == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) pW3[c * PE_WIDTH + f] = vW3[c];
    pb1[f] = sb1;
    pb2[f] = sb2;
    if (w == 0 && j < 3) pb3[j] = sgz;
  }
}

// sum of the per-workgroup partials [n_parts][n] -> out [n]; blockIdx.y takes a slice of the parts, slices meet in
// `out` (zeroed by the caller) with one float atomic per element
#define PE_REDUCE_SLICES 16
__global__ void __launch_bounds__(256)
pe_reduce_kernel(const float* __restrict__ part, int n_parts, int n, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int per = (n_parts + PE_REDUCE_SLICES - 1) / PE_REDUCE_SLICES;
  const int p0 = blockIdx.y * per, p1 = min(n_parts, p0 + per);
  float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
  int p = p0;
  for (; p + 4 <= p1; p += 4) {
    a0 += part[(int64_t)p * n + i];
    a1 += part[(int64_t)(p + 1) * n + i];
    a2 += part[(int64_t)(p + 2) * n + i];
    a3 += part[(int64_t)(p + 3) * n + i];
  }
  for (; p < p1; ++p) a0 += part[(int64_t)p * n + i];
  if (p1 > p0) atomicAdd(out + i, (a0 + a1) + (a2 + a3));
}

static bool pe_shape_ok(int width, int P, int E, int d_in) {
  return width == PE_WIDTH && P >= 1 && P <= PE_MAX_FREQ && E >= 0 && d_in == 3 + 6 * P + E && d_in <= PE_MAX_DIN;
}

extern "C" {

int dvgo_march_positions(const float* rays_start, const float* rays_dir, const int64_t* ray_id, const int64_t* step_id,
                         int64_t M, float stepdist, float* pts, void* stream) {
  if (M < 0) return DVGO_EINVAL;
  if (M == 0) return 0;
  if (!rays_start || !rays_dir || !ray_id || !step_id || !pts) return DVGO_EINVAL;
  if (!dvgo_fits(M)) return DVGO_ERANGE;
  pe_positions_kernel<<<dvgo_blocks(M, DVGO_BLOCK), DVGO_BLOCK, 0, (hipStream_t)stream>>>(rays_start, rays_dir, ray_id,
                                                                                        step_id, M, stepdist, pts);
  DVGO_LAUNCH_CHECK();
  return 0;
}

int dvgo_shade_pe_fwd(const float* pts, const float* freq, int P, const float* emb, int E, const int64_t* ray_id, int64_t M,
                      const float* W1, const float* b1, const float* W2, const float* b2, const float* W3, const float* b3,
                      int width, int d_in, float* rgb, float* H1, float* H2, uint64_t* masks, void* stream) {
  if (M < 0 || P < 0 || E < 0) return DVGO_EINVAL;
  if (!pe_shape_ok(width, P, E, d_in)) return DVGO_ERANGE;
  if (M == 0) return 0;
  if (!pts || !freq || !emb || !ray_id || !W1 || !b1 || !W2 || !b2 || !W3 || !b3 || !rgb) return DVGO_EINVAL;
  if ((H1 == nullptr) != (H2 == nullptr) || (H1 == nullptr) != (masks == nullptr)) return DVGO_EINVAL;
  const int64_t n_tiles = (M + 31) / 32;
  const int64_t want = (n_tiles + PE_WAVES - 1) / PE_WAVES;
  const int blocks = (int)(want < 256 ? want : 256);        // one workgroup per CU (LDS)
  pe_fwd_kernel<<<blocks, PE_THREADS, 0, (hipStream_t)stream>>>(pts, freq, P, emb, E, ray_id, M, W1, b1, W2, b2, W3, b3, d_in,
                                                              rgb, H1, H2, (unsigned long long*)masks);
  DVGO_LAUNCH_CHECK();
  return 0;
}

int dvgo_shade_pe_bwd(const float* g_rgb, const float* rgb, const uint64_t* masks, int64_t M, const float* W2,
                      const float* W3, int width, float* G1, float* gz, void* stream) {
  if (M < 0) return DVGO_EINVAL;
  if (width != PE_WIDTH) return DVGO_ERANGE;
  if (M == 0) return 0;
  if (!g_rgb || !rgb || !masks || !W2 || !W3 || !G1 || !gz) return DVGO_EINVAL;
  const int64_t n_tiles = (M + 31) / 32;
  const int64_t want = (n_tiles + PE_WAVES - 1) / PE_WAVES;
  const int blocks = (int)(want < 256 ? want : 256);
  pe_bwd_kernel<<<blocks, PE_THREADS, 0, (hipStream_t)stream>>>(g_rgb, rgb, (const unsigned long long*)masks, M, W2, W3, G1, gz);
  DVGO_LAUNCH_CHECK();
  return 0;
}

int64_t dvgo_shade_pe_record_size(int width, int d_in) {
  return (int64_t)width * width + (int64_t)width * d_in + 5 * (int64_t)width + 3;
}

int dvgo_shade_pe_wgrad(const float* G1, const float* gz, const uint64_t* masks, const float* W3, const float* H1,
                        const float* H2, const float* pts, const float* freq, int P, const float* emb, int E,
                        const int64_t* ray_id, int64_t M, int width, int d_in, int n_parts, float* part, float* total,
                        void* stream) {
  if (M < 0 || n_parts <= 0 || P < 0 || E < 0) return DVGO_EINVAL;
  if (!pe_shape_ok(width, P, E, d_in)) return DVGO_ERANGE;
  const int rec = (int)dvgo_shade_pe_record_size(width, d_in);
  hipStream_t s = (hipStream_t)stream;
  if (M == 0) {   // an empty batch: its arrays are empty, so their pointers may be null; the gradients are zeros
    if (!total) return DVGO_EINVAL;
    DVGO_HIP_TRY(hipMemsetAsync(total, 0, (size_t)rec * sizeof(float), s));
    return 0;
  }
  if (!G1 || !gz || !masks || !W3 || !H1 || !H2 || !pts || !freq || !emb || !ray_id || !part || !total) return DVGO_EINVAL;
  pe_wgrad_kernel<<<n_parts, PE_WG_THREADS, 0, s>>>(G1, gz, (const unsigned long long*)masks, W3, H1, H2, pts, freq, P, emb, E,
                                                   ray_id, M, d_in, rec, part);
  DVGO_LAUNCH_CHECK();
  DVGO_HIP_TRY(hipMemsetAsync(total, 0, (size_t)rec * sizeof(float), s));
  pe_reduce_kernel<<<dim3((rec + 255) / 256, PE_REDUCE_SLICES), 256, 0, s>>>(part, n_parts, rec, total);
  DVGO_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
