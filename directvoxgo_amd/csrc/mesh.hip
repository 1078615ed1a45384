// Surface mesh of a trained scene: marching tetrahedra on the Freudenthal (Kuhn) split of an extraction lattice
// (extends the reference's debug exports, run.py:514-553 and tools/vis_volume.py, from voxel dumps to a mesh).
//
// The lattice is R = (Rx, Ry, Rz) points, padded by one EMPTY point on every side: P = R + 2 per axis, points in the
// linear order (i * Py + j) * Pz + k of the padded lattice (z contiguous, as density's innermost axis).  A point is
// INSIDE when its field value f > iso (strict).  Every tetrahedron edge runs from a point p to p + e for one of seven
// directions e, in this order: x, y, z, xy, xz, yz, xyz, so a surface vertex is named by (point, direction):
//   vertex id = vbase[p] + popcount(mask[p] & ((1 << d) - 1))
// with mask[p] the 7-bit crossing mask of p and vbase the exclusive scan of popcount(mask) in point order.  Cell p (its
// lower corner) is split into 6 tetrahedra {p, p + e_a, p + e_a + e_b, p + (1,1,1)}, one per axis permutation (a, b, c)
// in the order xyz, xzy, yxz, yzx, zxy, zyx; faces are emitted in cell order, then tetrahedron order, then triangle order.
//
// Launches (no atomics; the output order is a function of the field alone):
//   mesh_field_kernel          padded field: copy of the density grid, or its trilinear sample at g = a + i * s (the
//                              corner weights of common.h), with the renderer's occupancy-mask lookup; padding and
//                              masked-out points get iso - 1
//   mesh_count_kernel          per point the crossing mask (stored, 1 byte) and per cell its triangle count, both summed
//                              per workgroup (stored: 2 words per workgroup)
//   mesh_scan_kernel           one workgroup: exclusive scan of the workgroup sums (scan.h), totals (V, F) at the end
//   mesh_emit_vertices_kernel  each workgroup re-derives its points' offsets from its base and writes position + normal
//   mesh_emit_faces_kernel     each workgroup re-derives its cells' face offsets and the vertex bases of the four lattice
//                              rows its cells touch (LDS), and writes the triangles
//
// Every arithmetic step is written in a fixed order and the library is built with -ffp-contract=off, so a CPU statement
// of the same steps in fp32 (tests/mesh_oracle.py) reproduces positions to rounding and ids exactly.
#include "common.h"
#include "scan.h"

#define MESH_B 256

// direction d (0..6) -> corner-offset bits (bit2 = +x, bit1 = +y, bit0 = +z): x=4, y=2, z=1, xy=6, xz=5, yz=3, xyz=7
__device__ __forceinline__ int mesh_dir_bits(int d) {
  constexpr unsigned P = 4u | (2u << 3) | (1u << 6) | (6u << 9) | (5u << 12) | (3u << 15) | (7u << 18);
  return (int)((P >> (3 * d)) & 7u);
}
// corner-offset bits (1..7) -> direction d
__device__ __forceinline__ int mesh_bits_dir(int b) {
  constexpr unsigned Q = (2u << 3) | (1u << 6) | (5u << 9) | (0u << 12) | (4u << 15) | (3u << 18) | (6u << 21);
  return (int)((Q >> (3 * b)) & 7u);
}

struct MeshDims {
  int Px, Py, Pz;
  int64_t n;        // Px * Py * Pz
  int64_t sX, sY;   // Py * Pz, Pz
};

static MeshDims mesh_dims(int Px, int Py, int Pz) {
  MeshDims D;
  D.Px = Px; D.Py = Py; D.Pz = Pz;
  D.sY = Pz; D.sX = (int64_t)Py * Pz; D.n = (int64_t)Px * D.sX;
  return D;
}

__device__ __forceinline__ int64_t mesh_corner_off(const MeshDims& D, int c) {
  return ((c >> 2) & 1) * D.sX + ((c >> 1) & 1) * D.sY + (c & 1);
}

// exclusive prefix of v over the 256 threads of the workgroup, and the workgroup total
__device__ __forceinline__ uint32_t mesh_block_excl(uint32_t v, uint32_t* s_w, uint32_t& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(inc, d);
    if (lane >= d) inc += o;
  }
  __syncthreads();                                  // s_w may still be read by a previous call
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  uint32_t pre = 0;
#pragma unroll
  for (int w = 0; w < MESH_B / 64; ++w) pre += (w < wave) ? s_w[w] : 0u;
  total = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
  return pre + inc - v;
}

// the 8 corners of the cell at point idx (corner c = bit2 +x, bit1 +y, bit0 +z) as an inside bit mask over c;
// corners outside the padded lattice read as outside (they only occur for points on the upper faces)
__device__ __forceinline__ unsigned mesh_corners_inside(const float* __restrict__ f, const MeshDims& D, int64_t idx,
                                                        int pi, int pj, int pk, float iso) {
  unsigned in = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const bool ok = (pi + ((c >> 2) & 1) < D.Px) & (pj + ((c >> 1) & 1) < D.Py) & (pk + (c & 1) < D.Pz);
    const float v = ok ? f[idx + mesh_corner_off(D, c)] : 0.0f;
    in |= (ok && v > iso) ? (1u << c) : 0u;
  }
  return in;
}

// tetrahedron t (0..5) of a cell: corner bits of its second and third corner (the first is 0, the last 7)
__device__ __forceinline__ int mesh_tet_c1(int t) { return (int)((0x112244u >> (4 * t)) & 0xfu); }
__device__ __forceinline__ int mesh_tet_c2(int t) { return (int)((0x353656u >> (4 * t)) & 0xfu); }
// (t: 0 xyz -> 4,6   1 xzy -> 4,5   2 yxz -> 2,6   3 yzx -> 2,3   4 zxy -> 1,5   5 zyx -> 1,3; nibbles low to high)

__device__ __forceinline__ int mesh_tet_tris(unsigned in, int t) {
  const unsigned m = 1u | (1u << mesh_tet_c1(t)) | (1u << mesh_tet_c2(t)) | 0x80u;
  const int n = __popc(in & m);
  return n == 2 ? 2 : (n & 1);
}

__device__ __forceinline__ void mesh_point_ijk(const MeshDims& D, int64_t idx, int& pi, int& pj, int& pk) {
  pi = (int)(idx / D.sX);
  const int64_t r = idx - (int64_t)pi * D.sX;
  pj = (int)(r / D.sY);
  pk = (int)(r - (int64_t)pj * D.sY);
}

struct MeshFieldArgs {
  int X, Y, Z;                 // density grid
  int MX, MY, MZ;              // occupancy mask grid (mask may be null: all occupied)
  float msc[3], msh[3];        // mask xyz -> ijk scale / shift (MaskCache.xyz2ijk_*)
  int Rx, Ry, Rz;              // unpadded lattice
  float a[3], s[3];            // grid-index coordinate of lattice point i: a + i * s
  float mn[3], h[3];           // world position of lattice point i: mn + i * h
  int copy;                    // lattice == density grid: g = i, the value is read, not interpolated
  float iso;
};

__global__ void __launch_bounds__(MESH_B)
mesh_field_kernel(const float* __restrict__ density, const uint8_t* __restrict__ mask, MeshDims D, MeshFieldArgs A,
                  float* __restrict__ field) {
  const int64_t idx = (int64_t)blockIdx.x * MESH_B + threadIdx.x;
  if (idx >= D.n) return;
  int pi, pj, pk;
  mesh_point_ijk(D, idx, pi, pj, pk);
  const int i = pi - 1, j = pj - 1, k = pk - 1;
  const float empty = A.iso - 1.0f;
  float v = empty;
  bool in = (i >= 0) & (i < A.Rx) & (j >= 0) & (j < A.Ry) & (k >= 0) & (k < A.Rz);
  if (in && mask) {            // the renderer's lookup (pointwise.hip, K8): roundf(fmaf(xyz, scale, shift)), half away from 0
    const float px = A.mn[0] + (float)i * A.h[0];
    const float py = A.mn[1] + (float)j * A.h[1];
    const float pz = A.mn[2] + (float)k * A.h[2];
    const int mi = (int)roundf(fmaf(px, A.msc[0], A.msh[0]));
    const int mj = (int)roundf(fmaf(py, A.msc[1], A.msh[1]));
    const int mk = (int)roundf(fmaf(pz, A.msc[2], A.msh[2]));
    in = (mi >= 0) & (mi < A.MX) & (mj >= 0) & (mj < A.MY) & (mk >= 0) & (mk < A.MZ);
    in = in && mask[((int64_t)mi * A.MY + mj) * A.MZ + mk];
  }
  if (in) {
    if (A.copy) {
      v = density[((int64_t)i * A.Y + j) * A.Z + k];
    } else {
      const TriSetup t = dvgo_tri_from_g(A.a[0] + (float)i * A.s[0], A.a[1] + (float)j * A.s[1], A.a[2] + (float)k * A.s[2]);
      v = dvgo_tri_value_c1(density, t, A.X, A.Y, A.Z);
    }
  }
  field[idx] = v;
}

__global__ void __launch_bounds__(MESH_B)
mesh_count_kernel(const float* __restrict__ f, MeshDims D, float iso, uint8_t* __restrict__ edge_mask,
                  uint32_t* __restrict__ partials) {
  __shared__ uint32_t s_w[MESH_B / 64];
  const int64_t idx = (int64_t)blockIdx.x * MESH_B + threadIdx.x;
  uint32_t nv = 0, nf = 0;
  if (idx < D.n) {
    int pi, pj, pk;
    mesh_point_ijk(D, idx, pi, pj, pk);
    const unsigned in = mesh_corners_inside(f, D, idx, pi, pj, pk, iso);
    unsigned m = 0;
#pragma unroll
    for (int d = 0; d < 7; ++d) {
      const int b = mesh_dir_bits(d);
      const bool ok = (pi + ((b >> 2) & 1) < D.Px) & (pj + ((b >> 1) & 1) < D.Py) & (pk + (b & 1) < D.Pz);
      m |= (ok && (((in >> b) ^ in) & 1u)) ? (1u << d) : 0u;
    }
    edge_mask[idx] = (uint8_t)m;
    nv = __popc(m);
    if ((pi < D.Px - 1) & (pj < D.Py - 1) & (pk < D.Pz - 1)) {
#pragma unroll
      for (int t = 0; t < 6; ++t) nf += mesh_tet_tris(in, t);
    }
  }
  uint32_t tv, tf;
  mesh_block_excl(nv, s_w, tv);
  mesh_block_excl(nf, s_w, tf);
  if (threadIdx.x == 0) {
    partials[2 * (int64_t)blockIdx.x] = tv;
    partials[2 * (int64_t)blockIdx.x + 1] = tf;
  }
}

// bases[2w], bases[2w+1]: vertices / faces before workgroup w; bases[2W], bases[2W+1]: the totals V, F.
// V <= 7 * 2^28 and F <= 12 * 2^28 (the lattice bound of the entry point): both fit their 32-bit halves.
__global__ void __launch_bounds__(1024)
mesh_scan_kernel(const uint32_t* __restrict__ partials, int W, uint32_t* __restrict__ bases) {
  const unsigned long long total = block_scan_u64<16>(
      W, [&](int i) { return (unsigned long long)partials[2 * i] | ((unsigned long long)partials[2 * i + 1] << 32); },
      [&](int i, unsigned long long ex, unsigned long long) {
        bases[2 * i] = (uint32_t)ex;
        bases[2 * i + 1] = (uint32_t)(ex >> 32);
      });
  if (threadIdx.x == 0) {
    bases[2 * W] = (uint32_t)total;
    bases[2 * W + 1] = (uint32_t)(total >> 32);
  }
}

// central difference of the padded field at point (pi, pj, pk), indices clamped, each axis over its spacing
__device__ __forceinline__ void mesh_grad(const float* __restrict__ f, const MeshDims& D, int pi, int pj, int pk,
                                          const float* h, float& gx, float& gy, float& gz) {
  const int64_t b = (int64_t)pi * D.sX + (int64_t)pj * D.sY + pk;
  const int64_t xp = (pi + 1 < D.Px) ? D.sX : 0, xm = (pi > 0) ? D.sX : 0;
  const int64_t yp = (pj + 1 < D.Py) ? D.sY : 0, ym = (pj > 0) ? D.sY : 0;
  const int64_t zp = (pk + 1 < D.Pz) ? 1 : 0, zm = (pk > 0) ? 1 : 0;
  gx = (f[b + xp] - f[b - xm]) / h[0];
  gy = (f[b + yp] - f[b - ym]) / h[1];
  gz = (f[b + zp] - f[b - zm]) / h[2];
}

struct MeshBox {
  float mn[3], h[3];
};

__global__ void __launch_bounds__(MESH_B)
mesh_emit_vertices_kernel(const float* __restrict__ f, const uint8_t* __restrict__ edge_mask,
                          const uint32_t* __restrict__ bases, MeshDims D, float iso, MeshBox B, int64_t n_verts,
                          float* __restrict__ verts, float* __restrict__ normals) {
  __shared__ uint32_t s_w[MESH_B / 64];
  const int64_t idx = (int64_t)blockIdx.x * MESH_B + threadIdx.x;
  const unsigned m = (idx < D.n) ? edge_mask[idx] : 0u;
  uint32_t tot;
  const uint32_t ex = mesh_block_excl(__popc(m), s_w, tot);
  if (!m) return;
  int pi, pj, pk;
  mesh_point_ijk(D, idx, pi, pj, pk);
  const int64_t vb = (int64_t)bases[2 * (int64_t)blockIdx.x] + ex;
  const float f0 = f[idx];
  float g0x, g0y, g0z;
  mesh_grad(f, D, pi, pj, pk, B.h, g0x, g0y, g0z);
  int n = 0;
  for (int d = 0; d < 7; ++d) {
    if (!((m >> d) & 1u)) continue;
    const int b = mesh_dir_bits(d);
    const int bx = (b >> 2) & 1, by = (b >> 1) & 1, bz = b & 1;
    const float f1 = f[idx + mesh_corner_off(D, b)];
    const float t = (iso - f0) / (f1 - f0);
    const int64_t v = vb + n++;
    if (v >= n_verts) return;
    verts[3 * v + 0] = B.mn[0] + ((float)(pi - 1) + t * (float)bx) * B.h[0];
    verts[3 * v + 1] = B.mn[1] + ((float)(pj - 1) + t * (float)by) * B.h[1];
    verts[3 * v + 2] = B.mn[2] + ((float)(pk - 1) + t * (float)bz) * B.h[2];
    float g1x, g1y, g1z;
    mesh_grad(f, D, pi + bx, pj + by, pk + bz, B.h, g1x, g1y, g1z);
    const float gx = g0x + t * (g1x - g0x), gy = g0y + t * (g1y - g0y), gz = g0z + t * (g1z - g0z);
    const float len = sqrtf((gx * gx + gy * gy) + gz * gz);
    normals[3 * v + 0] = len > 0.0f ? -gx / len : 0.0f;
    normals[3 * v + 1] = len > 0.0f ? -gy / len : 0.0f;
    normals[3 * v + 2] = len > 0.0f ? -gz / len : 0.0f;
  }
}

// corner c minus corner o as an integer vector, and the determinant of three such vectors
struct MeshV { int x, y, z; };
__device__ __forceinline__ MeshV mesh_sub(int c, int o) {
  return {((c >> 2) & 1) - ((o >> 2) & 1), ((c >> 1) & 1) - ((o >> 1) & 1), (c & 1) - (o & 1)};
}
__device__ __forceinline__ int mesh_det(MeshV u, MeshV v, MeshV w) {
  return u.x * (v.y * w.z - v.z * w.y) - u.y * (v.x * w.z - v.z * w.x) + u.z * (v.x * w.y - v.y * w.x);
}

__global__ void __launch_bounds__(MESH_B)
mesh_emit_faces_kernel(const float* __restrict__ f, const uint8_t* __restrict__ edge_mask,
                       const uint32_t* __restrict__ bases, MeshDims D, int W, float iso, int64_t n_faces,
                       int32_t* __restrict__ faces) {
  // vertex bases and crossing masks of the points [q0_r, q0_r + B] of the four lattice rows r = 2 dx + dy that the
  // cells [w B, w B + B) reach: q0_r = w B + dx sX + dy sY (the z neighbour is the next entry)
  __shared__ uint32_t s_vb[4][MESH_B + 1];
  __shared__ uint8_t s_mk[4][MESH_B + 1];
  __shared__ uint32_t s_w[MESH_B / 64];
  const int tid = threadIdx.x;
  const int64_t w0 = (int64_t)blockIdx.x * MESH_B;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t q0 = w0 + (r >> 1) * D.sX + (r & 1) * D.sY;
    const int64_t c = q0 / MESH_B;                 // the chunk (= counting workgroup) q0 falls in; [q0, q0 + B] is in c, c + 1
    const int64_t e = q0 - c * MESH_B;
    const int64_t p0 = c * MESH_B + 2 * tid;
    const unsigned m0 = (p0 < D.n) ? edge_mask[p0] : 0u, m1 = (p0 + 1 < D.n) ? edge_mask[p0 + 1] : 0u;
    uint32_t tot;
    const uint32_t ex = mesh_block_excl(__popc(m0) + __popc(m1), s_w, tot);
    const uint32_t vb = bases[2 * (c < W ? c : (int64_t)W)] + ex;
    const int64_t l0 = 2 * tid - e, l1 = l0 + 1;
    if (l0 >= 0 && l0 <= MESH_B) { s_vb[r][l0] = vb; s_mk[r][l0] = (uint8_t)m0; }
    if (l1 >= 0 && l1 <= MESH_B) { s_vb[r][l1] = vb + __popc(m0); s_mk[r][l1] = (uint8_t)m1; }
  }
  const int64_t idx = w0 + tid;
  unsigned in = 0;
  uint32_t nf = 0;
  if (idx < D.n) {
    int pi, pj, pk;
    mesh_point_ijk(D, idx, pi, pj, pk);
    if ((pi < D.Px - 1) & (pj < D.Py - 1) & (pk < D.Pz - 1)) {
      in = mesh_corners_inside(f, D, idx, pi, pj, pk, iso);
#pragma unroll
      for (int t = 0; t < 6; ++t) nf += mesh_tet_tris(in, t);
    }
  }
  uint32_t tot;
  const uint32_t ex = mesh_block_excl(nf, s_w, tot);   // (its barriers also publish s_vb / s_mk)
  if (!nf) return;
  int64_t o = (int64_t)bases[2 * (int64_t)blockIdx.x + 1] + ex;
  // vertex id of the tetrahedron edge from corner u to corner v (u a subset of v)
  auto vid = [&](int u, int v) -> int32_t {
    const int r = ((u >> 2) & 1) * 2 + ((u >> 1) & 1), l = tid + (u & 1);
    const int d = mesh_bits_dir(u ^ v);
    return (int32_t)(s_vb[r][l] + __popc((unsigned)s_mk[r][l] & ((1u << d) - 1u)));
  };
  auto emit = [&](int32_t a, int32_t b, int32_t c) {
    if (o < n_faces) {
      faces[3 * o + 0] = a; faces[3 * o + 1] = b; faces[3 * o + 2] = c;
    }
    ++o;
  };
  for (int t = 0; t < 6; ++t) {
    const unsigned T = 0u | ((unsigned)mesh_tet_c1(t) << 3) | ((unsigned)mesh_tet_c2(t) << 6) | (7u << 9);
    auto cor = [&](int k) { return (int)((T >> (3 * k)) & 7u); };   // tetrahedron corner k (0..3), ordered by inclusion
    unsigned b = 0;                                                   // inside bits over k
#pragma unroll
    for (int k = 0; k < 4; ++k) b |= ((in >> cor(k)) & 1u) << k;
    const int n = __popc(b);
    if (n == 0 || n == 4) continue;
    if (n & 1) {
      // the lone corner L (the inside one of n = 1, the outside one of n = 3) and the others A < B < C
      const unsigned lone = (n == 1) ? b : (~b & 0xfu);
      const int L = __ffs(lone) - 1;
      const int A = (L == 0) ? 1 : 0, B = (L <= 1) ? 2 : 1, C = (L <= 2) ? 3 : 2;
      const int cl = cor(L), ca = cor(A), cb = cor(B), cc = cor(C);
      // right-hand normal from inside to outside: away from L when L is inside
      const bool keep = (mesh_det(mesh_sub(ca, cl), mesh_sub(cb, cl), mesh_sub(cc, cl)) > 0) == (n == 1);
      auto e = [&](int K, int ck) { return K < L ? vid(ck, cl) : vid(cl, ck); };
      const int32_t va = e(A, ca), vbb = e(B, cb), vc = e(C, cc);
      if (keep) emit(va, vbb, vc); else emit(va, vc, vbb);
    } else {
      // inside a < b, outside c < d; quad (ac, ad, bd, bc), its right-hand normal along (c - a) when det(d-c, b-a, c-a) > 0
      const int a = __ffs(b) - 1, bb = 31 - __clz(b);
      const unsigned ob = ~b & 0xfu;
      const int c = __ffs(ob) - 1, d = 31 - __clz(ob);
      const int ca = cor(a), cbb = cor(bb), cc = cor(c), cd = cor(d);
      auto e = [&](int K0, int c0, int K1, int c1) { return K0 < K1 ? vid(c0, c1) : vid(c1, c0); };
      const int32_t ac = e(a, ca, c, cc), ad = e(a, ca, d, cd), bd = e(bb, cbb, d, cd), bc = e(bb, cbb, c, cc);
      const int s = mesh_det(mesh_sub(cd, cc), mesh_sub(cbb, ca), mesh_sub(cc, ca));
      const int32_t q0 = ac, q1 = s > 0 ? ad : bc, q2 = bd, q3 = s > 0 ? bc : ad;
      if (min(q0, q2) < min(q1, q3)) {
        emit(q0, q1, q2); emit(q0, q2, q3);
      } else {
        emit(q0, q1, q3); emit(q1, q2, q3);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------------
#define MESH_MAX_POINTS ((int64_t)1 << 28)

static int mesh_check_dims(int Px, int Py, int Pz) {
  if (Px < 3 || Py < 3 || Pz < 3) return DVGO_EINVAL;   // a padded lattice has at least one real point per axis
  if ((int64_t)Px * Py * Pz > MESH_MAX_POINTS) return DVGO_ERANGE;
  return 0;
}

int dvgo_mesh_field(const float* density, int X, int Y, int Z, const uint8_t* mask, int MX, int MY, int MZ,
                    const float* mask_scale, const float* mask_shift, int Rx, int Ry, int Rz, const float* g0,
                    const float* gs, const float* box_min, const float* spacing, int copy, float iso, float* field,
                    void* stream) {
  if (X < 2 || Y < 2 || Z < 2 || Rx < 1 || Ry < 1 || Rz < 1) return DVGO_EINVAL;
  if ((int64_t)X * Y * Z >= ((int64_t)1 << 31)) return DVGO_ERANGE;
  const int rc = mesh_check_dims(Rx + 2, Ry + 2, Rz + 2);
  if (rc) return rc;
  if (!density || !g0 || !gs || !box_min || !spacing || !field) return DVGO_EINVAL;
  if (mask && (MX < 1 || MY < 1 || MZ < 1 || !mask_scale || !mask_shift)) return DVGO_EINVAL;
  if (copy && (Rx != X || Ry != Y || Rz != Z)) return DVGO_EINVAL;
  const MeshDims D = mesh_dims(Rx + 2, Ry + 2, Rz + 2);
  MeshFieldArgs A = {};
  A.X = X; A.Y = Y; A.Z = Z;
  A.MX = MX; A.MY = MY; A.MZ = MZ;
  A.Rx = Rx; A.Ry = Ry; A.Rz = Rz;
  for (int a = 0; a < 3; ++a) {
    A.msc[a] = mask ? mask_scale[a] : 0.f;
    A.msh[a] = mask ? mask_shift[a] : 0.f;
    A.a[a] = g0[a]; A.s[a] = gs[a]; A.mn[a] = box_min[a]; A.h[a] = spacing[a];
  }
  A.copy = copy ? 1 : 0;
  A.iso = iso;
  mesh_field_kernel<<<dvgo_blocks(D.n, MESH_B), MESH_B, 0, (hipStream_t)stream>>>(density, mask, D, A, field);
  DVGO_LAUNCH_CHECK();
  return 0;
}

int dvgo_mesh_count(const float* field, int Px, int Py, int Pz, float iso, uint8_t* edge_mask, uint32_t* partials,
                    uint32_t* bases, void* stream) {
  const int rc = mesh_check_dims(Px, Py, Pz);
  if (rc) return rc;
  if (!field || !edge_mask || !partials || !bases) return DVGO_EINVAL;
  const MeshDims D = mesh_dims(Px, Py, Pz);
  const int W = dvgo_blocks(D.n, MESH_B);
  hipStream_t s = (hipStream_t)stream;
  mesh_count_kernel<<<W, MESH_B, 0, s>>>(field, D, iso, edge_mask, partials);
  DVGO_LAUNCH_CHECK();
  mesh_scan_kernel<<<1, 1024, 0, s>>>(partials, W, bases);
  DVGO_LAUNCH_CHECK();
  return 0;
}

int dvgo_mesh_emit(const float* field, const uint8_t* edge_mask, const uint32_t* bases, int Px, int Py, int Pz,
                   float iso, const float* box_min, const float* spacing, int64_t n_verts, int64_t n_faces,
                   float* verts, float* normals, int32_t* faces, void* stream) {
  const int rc = mesh_check_dims(Px, Py, Pz);
  if (rc) return rc;
  if (n_verts < 0 || n_faces < 0) return DVGO_EINVAL;
  if (!field || !edge_mask || !bases || !box_min || !spacing) return DVGO_EINVAL;
  if ((n_verts > 0 && (!verts || !normals)) || (n_faces > 0 && !faces)) return DVGO_EINVAL;
  const MeshDims D = mesh_dims(Px, Py, Pz);
  const int W = dvgo_blocks(D.n, MESH_B);
  MeshBox B;
  for (int a = 0; a < 3; ++a) { B.mn[a] = box_min[a]; B.h[a] = spacing[a]; }
  hipStream_t s = (hipStream_t)stream;
  if (n_verts > 0) {
    mesh_emit_vertices_kernel<<<W, MESH_B, 0, s>>>(field, edge_mask, bases, D, iso, B, n_verts, verts, normals);
    DVGO_LAUNCH_CHECK();
  }
  if (n_faces > 0) {
    mesh_emit_faces_kernel<<<W, MESH_B, 0, s>>>(field, edge_mask, bases, D, W, iso, n_faces, faces);
    DVGO_LAUNCH_CHECK();
  }
  return 0;
}
