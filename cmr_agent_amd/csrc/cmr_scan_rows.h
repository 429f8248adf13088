// What the kernels that walk the rows of a raw scan [N][ld] share (voxel_map.hip: map_keys_kernel; voxel_map_rays.hip: map_rays_kernel;
// scan_descriptor.hip: scan_descriptor_kernel; range_image.hip: range_scatter_kernel), stated once: how a row comes in
// and when it is dropped, the azimuth bin of a direction, and the two ways a launch leaves its per-call counts.  What a kernel does with a
// row that came in -- its key, its ray, its ring, its image row -- and which rows it calls outside stay with the kernel.  Device code.
#pragma once
#include "cmr_cloud_grid.h"

constexpr int64_t ROW_LIMIT = (int64_t)1 << 31;                   // an entry point takes fewer rows than this: a row index fits 31 bits

// ---- row intake ----------------------------------------------------------------------------------------------------------------------------
// Row i as the kernel goes on with it: (x, y, z) as loaded, moved by the loaded pose T (pose_load) when `posed`.  -> the row is finite
// before AND after the pose step; a row that is not is `dropped`, and (x, y, z) are set all the same.  (map_rays_kernel states the same
// operations in its own opening: with this function there its walk measured 5 % slower)
__device__ __forceinline__ bool scan_row(const float* __restrict__ pts, int64_t ld, int64_t i, bool posed, const float (&T)[12], float& x,
                                         float& y, float& z) {
  const float px = pts[i * ld], py = pts[i * ld + 1], pz = pts[i * ld + 2];
  x = px, y = py, z = pz;
  if (posed) pose_apply(T, px, py, pz, x, y, z);
  return cmr_finite3(px, py, pz) && cmr_finite3(x, y, z);
}
// a scan in the sensor's own frame: no pose
__device__ __forceinline__ bool scan_row(const float* __restrict__ pts, int64_t ld, int64_t i, float& x, float& y, float& z) {
  const float none[12] = {};
  return scan_row(pts, ld, i, false, none, x, y, z);
}

// ---- the azimuth bin -----------------------------------------------------------------------------------------------------------------------
// The table of a circle cut into 4 `quarter` bins: (cos, sin) of the quarter - 1 bin edges inside the first quadrant, into LDS by a
// workgroup of 256; the caller's barrier follows.
__device__ __forceinline__ void azimuth_load(const float* __restrict__ dir, int quarter, float (*dirs)[2]) {
  for (int k = threadIdx.x; k < quarter - 1; k += 256) {
    dirs[k][0] = dir[2 * k];
    dirs[k][1] = dir[2 * k + 1];
  }
}
// The bin of direction (x, y), from the x axis towards y: the quadrant q by exact swaps and negations, inside it the number m of edges k
// with fp32(v c_k) >= fp32(u s_k), found by bisection -- c_k descends, s_k ascends, u, v >= 0 and an fp32 product is monotone in each
// factor, so the comparisons that hold are the first m (include/cmr_hip.h).  m is the lower end of a search over [0, quarter - 1] whatever
// the table holds: the bin lies in [0, 4 quarter).
__device__ __forceinline__ int azimuth_bin(float x, float y, const float (*dirs)[2], int quarter) {
#pragma clang fp contract(off)
  int q;
  float u, v;
  if (x > 0.f && y >= 0.f) {
    q = 0, u = x, v = y;
  } else if (x <= 0.f && y > 0.f) {
    q = 1, u = y, v = -x;
  } else if (x < 0.f && y <= 0.f) {
    q = 2, u = -x, v = -y;
  } else if (x >= 0.f && y < 0.f) {
    q = 3, u = -y, v = x;
  } else {
    q = 0, u = 0.f, v = 0.f;                                      // x = y = 0
  }
  int m = 0, end = quarter - 1;                                   // the comparisons below m hold, those from `end` on do not
  while (m < end) {
    const int mid = (m + end) >> 1;
    const float vc = v * dirs[mid][0], us = u * dirs[mid][1];
    if (vc >= us) m = mid + 1; else end = mid;
  }
  return q * quarter + m;
}

// ---- counts by atomics: a kernel whose workgroups take many rows each (scan_descriptor.hip, range_image.hip) ----------------------------------
// counts[0..2] += (binned, dropped, outside) of a workgroup of 256 that took `rows` rows: a sum per wave by shuffles, the four waves'
// through `part` (LDS) by thread 0, one integer add per count that is not 0.  Every thread calls it; the entry point has zeroed counts.
__device__ __forceinline__ void scan_counts_add(int dropped, int outside, int rows, int (&part)[2][4], unsigned long long* __restrict__ counts) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    dropped += __shfl_xor(dropped, o, 64);
    outside += __shfl_xor(outside, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    part[0][threadIdx.x >> 6] = dropped;
    part[1][threadIdx.x >> 6] = outside;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int d = part[0][0] + part[0][1] + part[0][2] + part[0][3], o = part[1][0] + part[1][1] + part[1][2] + part[1][3];
    if (rows - d - o) atomicAdd(&counts[0], (unsigned long long)(rows - d - o));
    if (d) atomicAdd(&counts[1], (unsigned long long)d);
    if (o) atomicAdd(&counts[2], (unsigned long long)o);
  }
}

// ---- counts by packed flags: a kernel of one row per lane that ends in scan256 anyway (voxel_map.hip, voxel_map_rays.hip) -----------------------
// A lane raises at most one flag; field f of its word is BITS wide and starts at bit f BITS.  scan256's total is the workgroup's word: a
// field holds at most 256, which takes 9 bits.  The fields are the counts in the order the entry point returns them.
enum { ROW_DROPPED, ROW_OUTSIDE, ROW_LONG };
constexpr int KEYS_FLAG_BITS = 16, RAYS_FLAG_BITS = 10;
template <int BITS>
constexpr int row_flag(int field) {
  return 1 << (BITS * field);
}
// The second stage, one workgroup: counts[REST + f] = the sum of field f over the workgroups' words, and with REST counts[0] = N less
// all of them (the rays' `cast`).  Internal linkage and a template for the reason cmr_reduce.h gives for its kernels.
template <int FIELDS, int BITS, bool REST>
static __global__ __launch_bounds__(256) void flag_counts_kernel(const int32_t* __restrict__ part, int64_t blocks, int64_t N,
                                                                 int64_t* __restrict__ counts) {
  static_assert(BITS >= 9 && (FIELDS - 1) * BITS + 9 <= 31, "every field holds 256 and the word stays positive");
  __shared__ int64_t sh[FIELDS][256];
  int64_t c[FIELDS] = {};
  for (int64_t b = threadIdx.x; b < blocks; b += 256) {
#pragma unroll
    for (int f = 0; f < FIELDS; ++f) c[f] += part[b] >> (BITS * f) & ((1 << BITS) - 1);
  }
#pragma unroll
  for (int f = 0; f < FIELDS; ++f) sh[f][threadIdx.x] = c[f];
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) {
#pragma unroll
      for (int f = 0; f < FIELDS; ++f) sh[f][threadIdx.x] += sh[f][threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    int64_t rest = N;
#pragma unroll
    for (int f = 0; f < FIELDS; ++f) {
      counts[REST + f] = sh[f][0];
      rest -= sh[f][0];
    }
    if (REST) counts[0] = rest;
  }
}
