// What a spinning LiDAR standing at a pose would see of a cloud (port extension): a spherical z-buffer, restated in
// include/cmr_hip.h so that every integer follows from stated fp32 operations -- no atan2, no sqrt, no fused multiply-add.
//
//   range_fill_kernel      the packed image = all ones and the three counts = 0, one 64-bit word per lane
//   range_scatter_kernel   1 024 rows per workgroup, one row per lane and pass, the pose loaded once ahead of the passes: the row's intake
//                          (cmr_scan_rows.h), the squares and the range test first (a row out of range costs its load and three
//                          products), then the image row by binary search in its table and the column as cmr_scan_rows.h's azimuth bin
//                          (both tables in LDS, 9 KiB) -- the comparisons are monotone in the table index, so a search gives the count
//                          the header states -- and the winner by ONE 64-bit unsigned atomic min on (bits(d2) << 32 | row index), skipped
//                          when a plain load of the cell already shows a key at or below the lane's (a cell only ever decreases); the
//                          three counts by cmr_scan_rows.h's shuffle sums and at most one integer atomic add per workgroup and count
//   range_unpack_kernel    index and dist2 of a packed cell, one cell per lane
//   range_visible_kernel   the windowed minimum of dist2 round a cell and the test against it, one cell per lane, plain stores
// A minimum of packed integers and an integer sum are order free, and every other output is a plain store by its owner: two calls agree
// bit for bit.  The image row is the lower end of a search interval inside [0, R] that never reaches R, the column q C / 4 + m with
// q <= 3 and m the lower end of a search over [0, C / 4 - 1], so the cell lies in [0, R C) whatever the rows and the tables hold; the
// window of the visible kernel is clipped to [0, R) and wrapped into [0, C): no store and no load leaves the arrays.
#include "cmr_scan_rows.h"

#include <math.h>

namespace {

constexpr int MAX_ROWS = 128, MAX_COLS = 4096, MAX_CELLS = 1 << 19;
constexpr int MAX_WINDOW = 1024;                                  // cells the visible kernel reads per cell at most
constexpr int SCATTER_ROWS = 1024;                                // rows per workgroup of the scatter kernel: four per lane
constexpr unsigned long long EMPTY = ~0ull;

__host__ __device__ inline bool shape_ok(int R, int C) {
  return R >= 1 && R <= MAX_ROWS && C >= 4 && C <= MAX_COLS && C % 4 == 0 && R * C <= MAX_CELLS;
}

__global__ __launch_bounds__(256) void range_fill_kernel(unsigned long long* __restrict__ image, int cells, unsigned long long* __restrict__ counts) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < cells) image[c] = EMPTY;
  if (c < 3) counts[c] = 0;
}

// elevation >= edge j, (s, q) = (sign of tan e_j, tan^2 e_j)
__device__ __forceinline__ bool above(float s, float q, float z, float zz, float r2) {
#pragma clang fp contract(off)
  const float rhs = r2 * q;
  return s > 0.f ? (z >= 0.f && zz >= rhs) : (s < 0.f ? (z >= 0.f || zz <= rhs) : z >= 0.f);
}

__global__ __launch_bounds__(256) void range_scatter_kernel(const float* __restrict__ pts, int64_t ld, int64_t N, const float* __restrict__ pose,
                                                            int R, int C, const float* __restrict__ elev_tab, const float* __restrict__ col_dir,
                                                            float min_range2, float max_range2, unsigned long long* image,
                                                            unsigned long long* __restrict__ counts) {
#pragma clang fp contract(off)
  __shared__ float elev[MAX_ROWS + 1][2];
  __shared__ float dirs[MAX_COLS / 4][2];
  __shared__ int part[2][4];
  const int quarter = C / 4;
  for (int j = threadIdx.x; j <= R; j += 256) {
    elev[j][0] = elev_tab[2 * j];
    elev[j][1] = elev_tab[2 * j + 1];
  }
  azimuth_load(col_dir, quarter, dirs);
  float T[12];
  if (pose) pose_load(pose, T);
  __syncthreads();
  int dropped = 0, outside = 0;
  const int64_t first = (int64_t)blockIdx.x * SCATTER_ROWS;
  for (int p = 0; p < SCATTER_ROWS / 256; ++p) {
    const int64_t i = first + p * 256 + threadIdx.x;
    if (i >= N) break;
    float x, y, z;
    if (!scan_row(pts, ld, i, pose != nullptr, T, x, y, z)) {
      ++dropped;
      continue;
    }
    const float xx = x * x, yy = y * y, zz = z * z;
    const float r2 = xx + yy;
    const float d2 = r2 + zz;
    if (d2 < min_range2 || d2 >= max_range2) {                    // a square may overflow: an infinite d2 is outside
      ++outside;
      continue;
    }
    if (!above(elev[0][0], elev[0][1], z, zz, r2) || above(elev[R][0], elev[R][1], z, zz, r2)) {
      ++outside;
      continue;
    }
    int row = 0, top = R;                                         // above(row) holds, above(top) does not; row < top <= R throughout
    while (top - row > 1) {
      const int mid = (row + top) >> 1;
      if (above(elev[mid][0], elev[mid][1], z, zz, r2)) row = mid; else top = mid;
    }
    const int cell = row * C + azimuth_bin(x, y, dirs, quarter);
    const unsigned long long key = (unsigned long long)__builtin_bit_cast(unsigned, d2) << 32 | (unsigned long long)i;      // d2 > 0: its bits order like it
    if (key < image[cell]) atomicMin(&image[cell], key);
  }
  scan_counts_add(dropped, outside, (int)(N - first < SCATTER_ROWS ? N - first : SCATTER_ROWS), part, counts);
}

__global__ __launch_bounds__(256) void range_unpack_kernel(const unsigned long long* __restrict__ image, int cells, int32_t* __restrict__ index,
                                                           float* __restrict__ dist2) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cells) return;
  const unsigned long long key = image[c];
  const bool empty = key == EMPTY;
  index[c] = empty ? -1 : (int32_t)(key & 0xffffffffull);
  dist2[c] = __builtin_bit_cast(float, empty ? 0x7fc00000u : (unsigned)(key >> 32));
}

// visible[r][c] = the cell has a winner and d2 <= fp32(m2 factor), m2 = the least dist2 over the window's cells that have one
__global__ __launch_bounds__(256) void range_visible_kernel(const float* __restrict__ dist2, int R, int C, int radius_rows, int span_cols,
                                                            int first_col, float factor, uint8_t* __restrict__ visible) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= R * C) return;
  const int r = t / C, c = t - r * C;
  const float d2 = dist2[t];
  bool seen = false;
  if (d2 == d2) {
    const int r0 = r - radius_rows > 0 ? r - radius_rows : 0, r1 = r + radius_rows < R - 1 ? r + radius_rows : R - 1;
    int c0 = c + first_col;                                       // first_col in (-C, 0]: the window's first column, wrapped
    c0 = c0 < 0 ? c0 + C : c0;
    float m2 = d2;
    for (int rr = r0; rr <= r1; ++rr) {
      int cc = c0;
      for (int k = 0; k < span_cols; ++k) {                       // span_cols <= C: no column twice
        const float o = dist2[rr * C + cc];
        m2 = o < m2 ? o : m2;                                     // a NaN (an empty cell) is never below
        cc = cc + 1 == C ? 0 : cc + 1;
      }
    }
    const float bound = m2 * factor;
    seen = d2 <= bound;
  }
  visible[t] = seen ? 1 : 0;
}

}  // namespace

extern "C" int64_t cmr_range_image_workspace_bytes(int rows, int cols) { return shape_ok(rows, cols) ? (int64_t)rows * cols * 8 : 0; }

extern "C" int cmr_range_image_f32(const float* points, int64_t ld, int64_t N, const float* pose, int rows, int cols, const float* elev,
                                   const float* col_dir, float min_range2, float max_range2, int32_t* index, float* dist2, int64_t* counts,
                                   void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  CMR_REQUIRE(points && ld >= 3 && N > 0 && N < ROW_LIMIT && rows >= 1 && cols >= 1 && elev && index && dist2 && counts && workspace &&
              cmr_aligned16(workspace));
  if (!shape_ok(rows, cols)) return CMR_EUNSUPPORTED;
  CMR_REQUIRE((cols == 4 || col_dir) && min_range2 > 0.f && min_range2 < max_range2 && isfinite(max_range2) &&
              workspace_bytes >= cmr_range_image_workspace_bytes(rows, cols));
  const int cells = rows * cols;
  unsigned long long* image = (unsigned long long*)workspace;
  hipLaunchKernelGGL(range_fill_kernel, dim3(blocks_of(cells, 256)), dim3(256), 0, stream, image, cells, (unsigned long long*)counts);
  hipLaunchKernelGGL(range_scatter_kernel, dim3(blocks_of(N, SCATTER_ROWS)), dim3(256), 0, stream, points, ld, N, pose, rows, cols, elev, col_dir,
                     min_range2, max_range2, image, (unsigned long long*)counts);
  hipLaunchKernelGGL(range_unpack_kernel, dim3(blocks_of(cells, 256)), dim3(256), 0, stream, image, cells, index, dist2);
  return cmr_launch_status();
}

extern "C" int cmr_range_visible_f32(const float* dist2, int rows, int cols, int radius_rows, int radius_cols, float factor, uint8_t* visible,
                                     hipStream_t stream) {
  CMR_REQUIRE(dist2 && visible && rows >= 1 && cols >= 1 && radius_rows >= 0 && radius_cols >= 0 && factor >= 1.f && isfinite(factor));
  if (!shape_ok(rows, cols)) return CMR_EUNSUPPORTED;
  const int span_rows = radius_rows < rows / 2 ? 2 * radius_rows + 1 : rows;          // the rows a clipped window holds at most
  const bool whole = radius_cols >= cols / 2;                     // 2 radius_cols + 1 > cols: every column of a row, once
  const int span_cols = whole ? cols : 2 * radius_cols + 1;
  CMR_REQUIRE((int64_t)span_rows * span_cols <= MAX_WINDOW);
  hipLaunchKernelGGL(range_visible_kernel, dim3(blocks_of(rows * cols, 256)), dim3(256), 0, stream, dist2, rows, cols,
                     radius_rows < rows ? radius_rows : rows, span_cols, whole ? 0 : -radius_cols, factor, visible);
  return cmr_launch_status();
}
