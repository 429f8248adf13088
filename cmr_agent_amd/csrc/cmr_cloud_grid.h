// The sorted-key uniform grid that the cloud kernels share (cloud_prepare.hip: keys and normals; cloud_icp.hip: nearest row
// and point-to-plane ICP; cloud_fpfh.hip: SPFH and FPFH), stated once: the cell of a coordinate, the key of a
// cell, the cells a fixed-radius query searches along an axis, the run of sorted rows behind a range of keys, the membership test -- and the
// index as the kernels take it (GridIndex), the cells round a row or a free query (Walk) and the one loop over them (walk16), DESIGN.md 4ag;
// and what else more than one cloud source states (voxel_map.hip): the fp32 pose step, the workgroup scan, the block count.
// Device code, and the host's check of a GridIndex.
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
// the cell of a cell coordinate t = cell_coord(..), and whether the grid has it: the test is on the float, so +-inf and 3e38 are outside
// like cell -1 (voxel_map.hip: a row's key; voxel_map_rays.hip: both ends of a ray)
__device__ __forceinline__ bool grid_cell(float t, int64_t& c) {
  const float f = floorf(t);
  const bool inside = f >= 0.f && f <= (float)CELL_MAX;
  c = inside ? (int64_t)f : 0;
  return inside;
}

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
// the squared distance, every operation rounded on its own, and the membership test on it
__device__ __forceinline__ float dist2(float dx, float dy, float dz) {
#pragma clang fp contract(off)
  return (dx * dx + dy * dy) + dz * dz;
}
__device__ __forceinline__ bool within(float dx, float dy, float dz, float r2) { return dist2(dx, dy, dz) <= r2; }
__device__ __forceinline__ int isum16(int s) {
  s += cmr_dpp<0xB1>(s);
  s += cmr_dpp<0x4E>(s);
  s += cmr_dpp<0x141>(s);
  s += cmr_dpp<0x140>(s);
  return s;
}

// ---- what the cloud sources share beside the grid ----------------------------------------------------------------------------------------
// a pose as the kernels apply it: R row-major, then t -- from the upper 3 x 4 of a row-major fp32 [4][4]
__device__ __forceinline__ void pose_load(const float* __restrict__ pose, float (&T)[12]) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) T[3 * r + c] = pose[4 * r + c];
    T[9 + r] = pose[4 * r + 3];
  }
}
// q = R p + t in fp32, every operation rounded on its own, left to right
__device__ __forceinline__ void pose_apply(const float (&T)[12], float px, float py, float pz, float& qx, float& qy, float& qz) {
#pragma clang fp contract(off)
  qx = ((T[0] * px + T[1] * py) + T[2] * pz) + T[9];
  qy = ((T[3] * px + T[4] * py) + T[5] * pz) + T[10];
  qz = ((T[6] * px + T[7] * py) + T[8] * pz) + T[11];
}
// exclusive scan of one int per thread over the workgroup of 256 (Hillis-Steele in LDS); `total` is the workgroup's sum
__device__ __forceinline__ int scan256(int v, int (&buf)[256], int& total) {
  const int t = threadIdx.x;
  buf[t] = v;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const int a = t >= off ? buf[t - off] : 0;
    __syncthreads();
    buf[t] += a;
    __syncthreads();
  }
  const int incl = buf[t];
  total = buf[255];
  __syncthreads();
  return incl - v;
}
static inline unsigned blocks_of(int64_t items, int per_block) { return (unsigned)((items + per_block - 1) / per_block); }

// ---- the index ---------------------------------------------------------------------------------------------------------------------------
// A grid index as ops.cloud_index builds it, passed to the kernels by value: the kept rows as float4 in key order, their sorted keys, their
// original row numbers, and the grid the keys were taken on.
struct GridIndex {
  const f32x4* __restrict__ pts4;
  const int64_t* __restrict__ keys;
  const int64_t* __restrict__ order;
  int64_t kept;
  float ox, oy, oz, cell;
};
// the host's check of an index; what an entry point asks on top of it (radius <= cell, max_dist <= cell, kept <= N) stays with the entry point
static inline bool grid_index_ok(const GridIndex& g) {
  return g.pts4 && g.keys && g.order && cmr_aligned16(g.pts4) && g.kept > 0 && g.kept < ((int64_t)1 << 31) && isfinite(g.ox) && isfinite(g.oy) &&
         isfinite(g.oz) && g.cell > 0.f && isfinite(g.cell);
}

// The cells of the grid that a FREE query searches along one axis.  A query inside the grid: axis_cells.  A query outside it has no
// cell of its own; up to two cells below cell 0 (above CELL_MAX) it can still reach cell 0 and, from a face, cell 1 -- both are searched,
// the distance test decides -- and beyond that nothing: lo > hi, no runs.  No index outside [0, CELL_MAX] leaves this function.
__device__ __forceinline__ void query_cells(float x, float origin, float cell, int& lo, int& hi) {
  const float c = floorf(cell_coord(x, origin, cell));
  if (c >= 0.f && c <= (float)CELL_MAX) {
    axis_cells(x, origin, cell, lo, hi);
  } else if (c >= -2.f && c < 0.f) {
    lo = 0;
    hi = 1;
  } else if (c > (float)CELL_MAX && c <= (float)(CELL_MAX + 2)) {
    lo = (int)CELL_MAX - 1;
    hi = (int)CELL_MAX;
  } else {                                                        // far outside, or not a number
    lo = 1;
    hi = 0;
  }
}

// the run of sorted rows behind the cells [xlo, xhi] of one (y, z) pair
__device__ __forceinline__ void cell_run(const int64_t* __restrict__ keys, int64_t kept, int xlo, int xhi, int yy, int zz, int64_t& b, int64_t& e) {
  b = key_bound(keys, kept, pack_key(xlo, yy, zz), false);
  e = b + key_bound(keys + b, kept - b, pack_key(xhi, yy, zz), true);
}

// ---- the walk ----------------------------------------------------------------------------------------------------------------------------
// The cells a 16-lane group searches, uniform over the group.  The cells of a (z, y) pair are consecutive along x, i.e. ONE range of keys
// and, the rows being sorted, one run of rows: nruns = ny * nz of them, 9 for a query inside a cell, up to 16 for one on a cell face (where
// axis_cells adds a cell on one side of an axis), 20 or 25 only beyond some 2^18 cells from the origin, where the rounding of cell_coord
// reaches half a cell and both sides are added.  `live` = false gives no runs.
struct Walk {
  int xlo, xhi, ylo, ny, zlo, nruns;
  // round a row of the cloud itself: it lies inside the grid
  __device__ __forceinline__ Walk(const f32x4& p, bool live, const GridIndex& g) {
    int yhi, zhi;
    axis_cells(p.x, g.ox, g.cell, xlo, xhi);
    axis_cells(p.y, g.oy, g.cell, ylo, yhi);
    axis_cells(p.z, g.oz, g.cell, zlo, zhi);
    ny = yhi - ylo + 1;
    nruns = live ? ny * (zhi - zlo + 1) : 0;
  }
  // round a free query, which may lie outside the grid (query_cells): no runs where an axis has no cells
  __device__ __forceinline__ Walk(float qx, float qy, float qz, bool live, const GridIndex& g) {
    int yhi, zhi;
    query_cells(qx, g.ox, g.cell, xlo, xhi);
    query_cells(qy, g.oy, g.cell, ylo, yhi);
    query_cells(qz, g.oz, g.cell, zlo, zhi);
    ny = yhi - ylo + 1;
    const int nz = zhi - zlo + 1;
    nruns = live && xhi >= xlo && ny > 0 && nz > 0 ? ny * nz : 0;
  }
};

// The walk of one 16-lane group: visit(j, pts4[j]) for every row j of every run, the runs in (z, y) order, lane l taking rows b + l, b + l +
// 16, ... of a run.  Lane r of the group finds run base + r with two binary searches, the group then reads every lane's (b, e) by shuffle.
// Entry conditions:
//   * EVERY lane of the wave calls it (the shuffles need every lane inside the loop), and is there again when it returns;
//   * w is uniform over the group -- nruns above all: a lane that left the loop early would be missing from the others' shuffles.
// One pass over `base`, save for the 20 or 25 runs far from the origin (above).  What happens to a visited row, the state it is added to and
// the 16-lane reduction after the walk are the caller's.  (g, w and the visitor go by value: taken by reference, spfh_kernel came out at
// 144 VGPRs instead of 128 and lost a wave per SIMD.)
template <typename Visit>
__device__ __forceinline__ void walk16(GridIndex g, Walk w, int lane, Visit visit) {
  for (int base = 0; base < w.nruns; base += 16) {
    int64_t b = 0, e = 0;                                           // lane r of the group finds run base + r
    if (base + lane < w.nruns) cell_run(g.keys, g.kept, w.xlo, w.xhi, w.ylo + (base + lane) % w.ny, w.zlo + (base + lane) / w.ny, b, e);
    const int here = w.nruns - base < 16 ? w.nruns - base : 16;
    for (int r = 0; r < here; ++r) {
      const int64_t rb = __shfl(b, r, 16), re = __shfl(e, r, 16);
      for (int64_t j = rb + lane; j < re; j += 16) visit(j, g.pts4[j]);
    }
  }
}
