// The sorted-key uniform grid that the cloud kernels share (cloud_prepare.hip: keys and normals; cloud_icp.hip: nearest row
// and point-to-plane ICP), stated once: the cell of a coordinate, the key of a cell, the cells a fixed-radius query
// searches along an axis, the run of sorted rows behind a range of keys, the membership test.  Device code only.
#pragma once
#include "cmr_common.h"

#include <math.h>

constexpr int CELL_BITS = 21;                                   // per axis; the key is cz << 42 | cy << 21 | cx
constexpr int64_t CELL_MAX = ((int64_t)1 << CELL_BITS) - 1;

// (x - origin) / cell: one IEEE subtraction, one IEEE division (hipcc divides fp32 correctly rounded by default; nothing here can contract)
__device__ __forceinline__ float cell_coord(float x, float origin, float cell) {
#pragma clang fp contract(off)
  const float d = x - origin;
  return d / cell;
}
// the cell index; the host has checked the cloud's bounds, the clamp only keeps a key well formed whatever it is handed
__device__ __forceinline__ int64_t cell_index(float x, float origin, float cell) {
  const float c = floorf(cell_coord(x, origin, cell));
  return c >= 0.f ? (c <= (float)CELL_MAX ? (int64_t)c : CELL_MAX) : 0;          // NaN -> 0
}
__device__ __forceinline__ int64_t pack_key(int64_t cx, int64_t cy, int64_t cz) { return cz << (2 * CELL_BITS) | cy << CELL_BITS | cx; }

// the cells a query searches along one axis: its own and one to either side -- and a second one on the side whose face the query sits on to
// within the rounding of cell_coord (a neighbour at distance radius there may round into the cell after next)
__device__ __forceinline__ void axis_cells(float x, float origin, float cell, int& lo, int& hi) {
  const float t = cell_coord(x, origin, cell);
  const float c = floorf(t);
  const float tol = (t + 2.f) * 9.5367431640625e-07f;           // 16 * 2^-24 (t + 2)
  const float frac = t - c;
  const int64_t ci = cell_index(x, origin, cell);
  const int64_t l = ci - 1 - (frac < tol ? 1 : 0), h = ci + 1 + (frac > 1.f - tol ? 1 : 0);
  lo = (int)(l < 0 ? 0 : l);
  hi = (int)(h > CELL_MAX ? CELL_MAX : h);
}
// first index in keys[0, n) whose key is >= k (upper = false) or > k (upper = true)
__device__ __forceinline__ int64_t key_bound(const int64_t* __restrict__ keys, int64_t n, int64_t k, bool upper) {
  int64_t lo = 0;
  while (n > 0) {
    const int64_t half = n >> 1;
    const int64_t v = keys[lo + half];
    if (upper ? v <= k : v < k) {
      lo += half + 1;
      n -= half + 1;
    } else {
      n = half;
    }
  }
  return lo;
}
__device__ __forceinline__ bool within(float dx, float dy, float dz, float r2) {
#pragma clang fp contract(off)
  return (dx * dx + dy * dy) + dz * dz <= r2;
}
__device__ __forceinline__ int isum16(int s) {
  s += cmr_dpp<0xB1>(s);
  s += cmr_dpp<0x4E>(s);
  s += cmr_dpp<0x141>(s);
  s += cmr_dpp<0x140>(s);
  return s;
}
