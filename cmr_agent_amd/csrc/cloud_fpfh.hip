// FPFH descriptors of a prepared cloud on the sorted-key grid (port extension): Open3D's ComputeFPFHFeature with a pure radius
// search, from the normals every prepared file carries.  The cloud is a grid index as ops.cloud_index builds it (cmr_cloud_grid.h), cell >=
// radius, so a row's neighbours lie in its own cell or one next to it; both kernels walk them with walk16 of cmr_cloud_grid.h: one 16-lane
// group per row in key order, one run of sorted rows per (z, y) pair of cells.
//
//   cmr_point_fpfh_f32   two launches on the caller's stream:
//     spfh_kernel   per row: its neighbours' pair features in fp64 (every operation rounded on its own), binned into 3 x 11 INTEGER counts --
//                   integer adds in LDS, order free and exact -- and the neighbour count k, into the workspace table (key order) and, when asked
//                   for, into the caller's spfh (row order);
//     fpfh_kernel   per row: sum over its neighbours of their SPFH value / d2 in fp64 -- every lane adds what it meets in sorted order, a
//                   balanced tree over the 16 lanes -- each group of 11 scaled to 100, the row's own SPFH value added, rounded to fp32.
// Every output has one writer; no floating-point atomics: two calls agree bit for bit.
#include "cmr_cloud_grid.h"

namespace {

constexpr int FP_BINS = 11;
constexpr int FP_DIM = 3 * FP_BINS;
constexpr int FP_GROUPS = 16;        // 16-lane groups (rows) per workgroup

// a row takes part when its normal is finite and not the zero vector
__device__ __forceinline__ bool takes_part(float nx, float ny, float nz) {
  return cmr_finite3(nx, ny, nz) && (nx != 0.f || ny != 0.f || nz != 0.f);
}

__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) {
#pragma clang fp contract(off)
  return (ax * bx + ay * by) + az * bz;
}
__device__ __forceinline__ int fp_bin(double x) {
#pragma clang fp contract(off)
  const double f = floor(11.0 * x);
  return f >= 10.0 ? 10 : (f >= 0.0 ? (int)f : 0);               // NaN -> 0
}

// The pair features of (p_i, n_i) and (p_j, n_j) in fp64 from the fp32 inputs, every operation rounded on its own.  false: the pair is skipped.
__device__ __forceinline__ bool pair_bins(const f32x4& pi, float nix, float niy, float niz, const f32x4& pj, float njx, float njy, float njz,
                                          int& b1, int& b2, int& b3) {
#pragma clang fp contract(off)
  double dx = (double)pj.x - (double)pi.x, dy = (double)pj.y - (double)pi.y, dz = (double)pj.z - (double)pi.z;
  const double len = sqrt(dot3(dx, dy, dz, dx, dy, dz));
  if (len == 0.0) return false;
  const double a1 = dot3(nix, niy, niz, dx, dy, dz) / len, a2 = dot3(njx, njy, njz, dx, dy, dz) / len;
  double n1x = nix, n1y = niy, n1z = niz, n2x = njx, n2y = njy, n2z = njz, f3 = a1;
  if (fabs(a1) < fabs(a2)) {
    n1x = njx, n1y = njy, n1z = njz, n2x = nix, n2y = niy, n2z = niz;
    dx = -dx, dy = -dy, dz = -dz;
    f3 = -a2;
  }
  double vx = dy * n1z - dz * n1y, vy = dz * n1x - dx * n1z, vz = dx * n1y - dy * n1x;
  const double vl = sqrt(dot3(vx, vy, vz, vx, vy, vz));
  if (vl == 0.0) return false;
  vx = vx / vl, vy = vy / vl, vz = vz / vl;
  const double wx = n1y * vz - n1z * vy, wy = n1z * vx - n1x * vz, wz = n1x * vy - n1y * vx;
  const double f2 = dot3(vx, vy, vz, n2x, n2y, n2z);
  const double f1 = atan2(dot3(wx, wy, wz, n2x, n2y, n2z), dot3(n1x, n1y, n1z, n2x, n2y, n2z));
  b1 = fp_bin((f1 + 3.141592653589793) / 6.283185307179586);
  b2 = fp_bin((f2 + 1.0) / 2.0);
  b3 = fp_bin((f3 + 1.0) / 2.0);
  return true;
}

// ------------------------------------------------------------------------------------------------------------------------------ SPFH
// table[q] (key order) = 33 counts, tcount[q] = k, or -1 for a row that takes no part.  Rows q in [kept, N) are the dropped ones: zeros.
__global__ __launch_bounds__(256) void spfh_kernel(GridIndex index, int64_t N, const float* __restrict__ normals, float radius,
                                                   int32_t* __restrict__ table, int32_t* __restrict__ tcount, int32_t* __restrict__ count,
                                                   int32_t* __restrict__ spfh) {
  __shared__ int hist[FP_GROUPS][FP_DIM];
  const int lane = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int64_t q = (int64_t)blockIdx.x * FP_GROUPS + g;
  for (int b = lane; b < FP_DIM; b += 16) hist[g][b] = 0;
  __syncthreads();
  const bool inidx = q < index.kept;
  const f32x4 p = index.pts4[inidx ? q : 0];
  const int64_t row = q < N ? index.order[q] : 0;
  const float nx = normals[row * 3], ny = normals[row * 3 + 1], nz = normals[row * 3 + 2];
  const bool live = inidx && takes_part(nx, ny, nz);
  const Walk w(p, live, index);
  const float r2 = radius * radius;
  int k = 0;
  walk16(index, w, lane, [&](int64_t j, const f32x4& c) {
    if (j == q) return;
    if (!within(c.x - p.x, c.y - p.y, c.z - p.z, r2)) return;
    const int64_t jr = index.order[j];
    const float mx = normals[jr * 3], my = normals[jr * 3 + 1], mz = normals[jr * 3 + 2];
    if (!takes_part(mx, my, mz)) return;
    ++k;
    int b1, b2, b3;
    if (pair_bins(p, nx, ny, nz, c, mx, my, mz, b1, b2, b3)) {
      atomicAdd(&hist[g][b1], 1);
      atomicAdd(&hist[g][FP_BINS + b2], 1);
      atomicAdd(&hist[g][2 * FP_BINS + b3], 1);
    }
  });
  k = isum16(k);
  asm volatile("" : "+v"(k));
  __syncthreads();
  if (q >= N) return;
  for (int b = lane; b < FP_DIM; b += 16) {
    const int v = hist[g][b];                                       // zero for a row that takes no part
    if (inidx) table[q * FP_DIM + b] = v;
    if (spfh) spfh[row * FP_DIM + b] = v;
  }
  if (lane != 0) return;
  if (inidx) tcount[q] = live ? k : -1;
  count[row] = k;
}

// ------------------------------------------------------------------------------------------------------------------------------ FPFH
__device__ __forceinline__ double spfh_value(int c, int k) {
#pragma clang fp contract(off)
  return (100.0 * (double)c) / (double)k;
}

__global__ __launch_bounds__(256) void fpfh_kernel(GridIndex index, int64_t N, float radius, const int32_t* __restrict__ table,
                                                   const int32_t* __restrict__ tcount, float* __restrict__ fpfh) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 15;
  const int64_t q = (int64_t)blockIdx.x * FP_GROUPS + (threadIdx.x >> 4);
  const bool inidx = q < index.kept;
  const f32x4 p = index.pts4[inidx ? q : 0];
  const int kq = inidx ? tcount[q] : -1;
  const Walk w(p, kq > 0, index);                                  // a row without neighbours has nothing to add
  const float r2 = radius * radius;
  double s[FP_DIM];
#pragma unroll
  for (int b = 0; b < FP_DIM; ++b) s[b] = 0.0;
  walk16(index, w, lane, [&](int64_t j, const f32x4& c) {
    if (j == q) return;
    const float dx = c.x - p.x, dy = c.y - p.y, dz = c.z - p.z;
    if (!within(dx, dy, dz, r2)) return;
    const float d2 = dist2(dx, dy, dz);
    const int kj = tcount[j];
    if (kj <= 0 || !(d2 > 0.f)) return;                             // takes no part (a neighbour of q has k >= 1: q itself), or d2 = 0
    const double D2 = (double)d2;
    const int32_t* t = table + j * FP_DIM;
#pragma unroll
    for (int bb = 0; bb < FP_DIM; ++bb) s[bb] += spfh_value(t[bb], kj) / D2;
  });
  // every lane of the wave is here again: the balanced tree over the 16 lanes
#pragma unroll
  for (int bb = 0; bb < FP_DIM; ++bb) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) s[bb] += __shfl_xor(s[bb], o, 16);
  }
  if (lane != 0 || q >= N) return;
  float* out = fpfh + index.order[q] * FP_DIM;
#pragma unroll
  for (int grp = 0; grp < 3; ++grp) {
    double tot = 0.0;
#pragma unroll
    for (int bb = 0; bb < FP_BINS; ++bb) tot += s[grp * FP_BINS + bb];
    const double scale = tot != 0.0 ? 100.0 / tot : 0.0;
#pragma unroll
    for (int bb = 0; bb < FP_BINS; ++bb) {
      const int e = grp * FP_BINS + bb;
      const double own = kq > 0 ? spfh_value(table[q * FP_DIM + e], kq) : 0.0;
      out[e] = (float)(s[e] * scale + own);
    }
  }
}

}  // namespace

extern "C" int64_t cmr_point_fpfh_workspace_bytes(int64_t kept) { return kept > 0 ? cmr_up16(kept * FP_DIM * 4) + cmr_up16(kept * 4) : 0; }

extern "C" int cmr_point_fpfh_f32(const float* points4, const int64_t* keys_sorted, const int64_t* order, int64_t N, int64_t kept, float ox,
                                  float oy, float oz, float cell, const float* normals, float radius, float* fpfh, int32_t* count,
                                  int32_t* spfh, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  const GridIndex index{(const f32x4*)points4, keys_sorted, order, kept, ox, oy, oz, cell};
  CMR_REQUIRE(grid_index_ok(index) && normals && fpfh && count && workspace && cmr_aligned16(workspace));
  CMR_REQUIRE(N > 0 && N < ((int64_t)1 << 31) && kept <= N && radius > 0.f && radius <= cell &&
              workspace_bytes >= cmr_point_fpfh_workspace_bytes(kept));
  int32_t* table = (int32_t*)workspace;
  int32_t* tcount = (int32_t*)((char*)workspace + cmr_up16(kept * FP_DIM * 4));
  const unsigned blocks = (unsigned)((N + FP_GROUPS - 1) / FP_GROUPS);
  hipLaunchKernelGGL(spfh_kernel, dim3(blocks), dim3(256), 0, stream, index, N, normals, radius, table, tcount, count, spfh);
  hipLaunchKernelGGL(fpfh_kernel, dim3(blocks), dim3(256), 0, stream, index, N, radius, (const int32_t*)table,
                     (const int32_t*)tcount, fpfh);
  return cmr_launch_status();
}
