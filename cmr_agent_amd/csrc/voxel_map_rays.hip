// Free space in a voxel map (port extension): every row of a scan is a beam from the sensor to its return, and the cells of
// the map's grid between the two were empty when it was taken.  One ray per lane walks those cells (Amanatides & Woo, stated on integers
// in include/cmr_hip.h so that every count is exact), looks each one up in the map's sorted keys and counts, per map row, the rays that
// passed through its voxel (crossed) and the rays that ended in it (hits).  Nothing in the map changes; the library keeps no state.
//
//   map_rays_kernel<RUNS>    the walk.  RUNS = false (the product's): every lookup is one key_bound over all M keys.  RUNS = true (A/B
//                            build only; it measured slower): while a ray steps along x its (y, z) pair stands still, and the cells of one
//                            pair are ONE run of the sorted keys -- the run behind the x cells the ray still has ahead of it is found once
//                            per pair and searched alone
// A row comes in by the operations cmr_scan_rows.h's scan_row states, written out here: the pose is loaded next to its use and the
// sensor taken from its shift in one branch, and the intake function in its place -- the same walk loop, laid out otherwise by the
// compiler -- measured 5 % slower.  The per-workgroup flag totals (that header's row_flag) become counts by its
// flag_counts_kernel<3, RAYS_FLAG_BITS, true>, one workgroup, as cmr_voxel_map_keys_f32 sums its two.
// crossed and hits are int32 sums by atomicAdd: order free, two calls agree exactly.  An index only ever comes out of a search over
// [0, M) that found an equal key there, so no store leaves crossed[0, M), hits[0, M) and counts whatever keys are handed over.
#include "cmr_cloud_grid.h"
#include "cmr_scan_rows.h"

namespace {

constexpr int MAX_CELLS_LIMIT = 65536;                          // the longest walk a lane can be asked for: bounds every lane's loop

// one axis of a ray: the cell coordinates of its ends, the cells they lie in, the steps still to make
struct RayAxis {
  float a, d;                                                     // a = cell_coord(o), d = cell_coord(q) - a
  int c, end, left, step;                                         // the cell the walk is in, the end's cell, |end - c|, sign(end - c)
};
__device__ __forceinline__ bool ray_axis(float o, float q, float origin, float cell, RayAxis& r) {
#pragma clang fp contract(off)
  const float a = cell_coord(o, origin, cell), b = cell_coord(q, origin, cell);
  int64_t s, e;
  const bool inside = grid_cell(a, s) & grid_cell(b, e);
  r.a = a;
  r.d = b - a;
  r.c = (int)s;
  r.end = (int)e;
  r.left = (int)(e > s ? e - s : s - e);
  r.step = e > s ? 1 : e < s ? -1 : 0;
  return inside;
}
// where the ray leaves the cell it is in along this axis, as a share of its length: recomputed from the integer cell, never accumulated;
// no division on an axis that has no step left (so d = 0 never divides)
__device__ __forceinline__ float ray_tmax(const RayAxis& r) {
#pragma clang fp contract(off)
  if (r.left == 0) return INFINITY;
  const float face = (float)(r.c + (r.step > 0 ? 1 : 0));
  const float num = face - r.a;
  return num / r.d;
}
__device__ __forceinline__ void ray_step(RayAxis& r, float& tmax) {
  r.c += r.step;
  --r.left;
  tmax = ray_tmax(r);
}

// the row of keys[lo, hi) that holds k, or -1
__device__ __forceinline__ int64_t find_key(const int64_t* __restrict__ keys, int64_t lo, int64_t hi, int64_t k) {
  const int64_t j = lo + key_bound(keys + lo, hi - lo, k, false);
  return j < hi && keys[j] == k ? j : -1;
}
// The run of sorted rows behind the cells [xlo, xhi] of one (y, z) pair: cell_run, with its second search cut short -- the keys being
// unique, the run holds at most xhi - xlo + 1 rows, and it is empty (the common case in free space) when the first row at or behind
// its first key already lies behind its last.  b <= e <= M whatever the keys are.
__device__ __forceinline__ void ray_run(const int64_t* __restrict__ keys, int64_t M, int xlo, int xhi, int cy, int cz, int64_t& b, int64_t& e) {
  const int64_t last = pack_key(xhi, cy, cz);
  b = key_bound(keys, M, pack_key(xlo, cy, cz), false);
  e = b;
  if (b < M && keys[b] <= last) {
    const int64_t span = (int64_t)(xhi - xlo) + 1;
    e = b + key_bound(keys + b, M - b < span ? M - b : span, last, true);
  }
}

template <bool RUNS>
__global__ __launch_bounds__(256) void map_rays_kernel(const float* __restrict__ pts, int64_t ld, int64_t N, const float* __restrict__ pose,
                                                       float ox, float oy, float oz, float cell, const int64_t* __restrict__ keys, int64_t M,
                                                       int start_margin, int end_margin, int max_cells, int32_t* __restrict__ crossed,
                                                       int32_t* __restrict__ hits, int32_t* __restrict__ part) {
  __shared__ int buf[256];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int flag = 0;
  if (i < N) {
    const float px = pts[i * ld], py = pts[i * ld + 1], pz = pts[i * ld + 2];
    float qx = px, qy = py, qz = pz, sx = 0.f, sy = 0.f, sz = 0.f;        // the end and the sensor
    if (pose) {
      float T[12];
      pose_load(pose, T);
      pose_apply(T, px, py, pz, qx, qy, qz);
      sx = T[9];
      sy = T[10];
      sz = T[11];
    }
    RayAxis x, y, z;
    if (!(cmr_finite3(px, py, pz) && cmr_finite3(qx, qy, qz))) {
      flag = row_flag<RAYS_FLAG_BITS>(ROW_DROPPED);
    } else if (!(ray_axis(sx, qx, ox, cell, x) & ray_axis(sy, qy, oy, cell, y) & ray_axis(sz, qz, oz, cell, z))) {
      flag = row_flag<RAYS_FLAG_BITS>(ROW_OUTSIDE);
    } else if (x.left + y.left + z.left > max_cells) {          // at most 3 (2^21 - 1): no overflow
      flag = row_flag<RAYS_FLAG_BITS>(ROW_LONG);
    } else {
      const int steps = x.left + y.left + z.left, lx = x.left, ly = y.left, lz = z.left;
      const int xlo = x.c < x.end ? x.c : x.end, xhi = x.c < x.end ? x.end : x.c;
      float tx = ray_tmax(x), ty = ray_tmax(y), tz = ray_tmax(z);
      int64_t rb = 0, re = 0;
      bool have_run = false;
      for (int n = 0; n < steps; ++n) {                            // steps <= max_cells <= 65 536
        // the cell the walk is in is not the end's: Chebyshev distances from the start's cell and to the end's
        const int ds = max(max(lx - x.left, ly - y.left), lz - z.left), de = max(max(x.left, y.left), z.left);
        if (ds > start_margin && de > end_margin) {
          const int64_t k = pack_key(x.c, y.c, z.c);
          int64_t j;
          if (RUNS && (have_run || x.left > 0)) {                  // a pair the ray only passes through in one cell: no run
            if (!have_run) {                                        // the x cells still ahead, this one included
              ray_run(keys, M, x.step > 0 ? x.c : xlo, x.step > 0 ? xhi : x.c, y.c, z.c, rb, re);
              have_run = true;
            }
            j = find_key(keys, rb, re, k);
          } else {
            j = find_key(keys, 0, M, k);
          }
          if (j >= 0) atomicAdd(&crossed[j], 1);
        }
        if (tx <= ty && tx <= tz) {                               // ties: x before y before z
          ray_step(x, tx);
        } else if (ty <= tz) {
          ray_step(y, ty);
          have_run = false;
        } else {
          ray_step(z, tz);
          have_run = false;
        }
      }
      const int64_t j = find_key(keys, 0, M, pack_key(x.c, y.c, z.c));      // the end's cell, whatever the rounding did on the way
      if (j >= 0) atomicAdd(&hits[j], 1);
    }
  }
  int total;
  scan256(flag, buf, total);
  if (threadIdx.x == 0) part[blockIdx.x] = total;
}

}  // namespace

// The product library searches the whole list: on the scan of tools/voxel_map_rays_bench.py the run-restricted lookup measured 0.67 x
// as fast.  It lives on in the A/B build alone (libcmr_hip_ab.so, include/cmr_hip_ab.h), for the tests that compare the
// two count by count and for that tool.
#ifdef CMR_AB_SWITCHES
static int g_rays_runs = 0;
extern "C" int cmr_set_voxel_map_rays_variant(int runs) {
  const int old = g_rays_runs;
  g_rays_runs = runs ? 1 : 0;
  return old;
}
#endif

extern "C" int64_t cmr_voxel_map_rays_workspace_bytes(int64_t N) { return N > 0 && N < ROW_LIMIT ? (N + 255) / 256 * 4 : 0; }

extern "C" int cmr_voxel_map_rays_f32(const int64_t* keys, int64_t M, float ox, float oy, float oz, float voxel, const float* points,
                                      int64_t ld, int64_t N, const float* pose, int start_margin, int end_margin, int max_cells,
                                      int32_t* crossed, int32_t* hits, int64_t* counts, void* workspace, int64_t workspace_bytes,
                                      hipStream_t stream) {
  CMR_REQUIRE(M >= 0 && M < ROW_LIMIT && (M == 0 || (keys && crossed && hits)) && points && ld >= 3 && N > 0 && N < ROW_LIMIT && counts &&
              workspace && voxel > 0.f && isfinite(voxel) && isfinite(ox) && isfinite(oy) && isfinite(oz) && start_margin >= 0 &&
              end_margin >= 0 && max_cells >= 1 && max_cells <= MAX_CELLS_LIMIT && workspace_bytes >= cmr_voxel_map_rays_workspace_bytes(N));
  if (M > 0 && (hipMemsetAsync(crossed, 0, (size_t)M * sizeof(int32_t), stream) != hipSuccess ||
                hipMemsetAsync(hits, 0, (size_t)M * sizeof(int32_t), stream) != hipSuccess))
    return CMR_ELAUNCH;
  const unsigned blocks = blocks_of(N, 256);
#ifdef CMR_AB_SWITCHES
  auto kernel = g_rays_runs ? map_rays_kernel<true> : map_rays_kernel<false>;
#else
  auto kernel = map_rays_kernel<false>;
#endif
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, stream, points, ld, N, pose, ox, oy, oz, voxel, keys, M, start_margin, end_margin,
                     max_cells, crossed, hits, (int32_t*)workspace);
  hipLaunchKernelGGL((flag_counts_kernel<3, RAYS_FLAG_BITS, true>), dim3(1), dim3(256), 0, stream, (const int32_t*)workspace, (int64_t)blocks, N,
                     counts);
  return cmr_launch_status();
}
