// A voxel map of registered scans (port extension): the rows of one scan, moved by its pose, are merged into a map that keeps
// one row per occupied voxel -- key, running mean of points and attributes, row count, the stamp of the last insert that touched it.  The map
// is a sorted unique key list; a scan becomes one too (the keys below, the caller's stable sort, cmr_segment_heads_i64 and
// cmr_segment_reduce_f32, as for the voxel downsample), and the merge is two sorted unique lists in and one out.
//
//   cmr_voxel_map_keys_f32    one pass over the scan's rows: the row's intake (cmr_scan_rows.h: q = R p + t, dropped or not), outside or
//                             the key, the moved row; the two counts from the workgroups' packed flags (cmr_scan_rows.h)
//   cmr_voxel_map_plan_i64    where every row of both sides goes: every scan voxel is located in the map's keys and every map row in the scan's
//                             by binary search, keep / miss / hit flags, their exclusive prefix sums (the tile scan of cloud_prepare.hip), sizes
//   (the caller reads the sizes back and allocates the new map)
//   cmr_voxel_map_write_f32   every output row by the one thread that owns it: a map row the scan missed is copied, one it hit is combined,
//                             a scan voxel the map lacks is copied in
// No re-sort of the map, no atomics, plain stores; every float result follows from operations stated one by one in include/cmr_hip.h.
#include "cmr_cloud_grid.h"
#include "cmr_scan_rows.h"

namespace {

constexpr int64_t KEY_DROPPED = -1;                             // a non-finite coordinate, before or after the pose
constexpr int64_t KEY_OUTSIDE = -2;                             // finite, but off the grid on some axis; both sort in front of every cell
                                                                // (a key takes all 63 bits: 2^63 - 1 is the last cell's)
constexpr int SCAN_TILE = 1024;                                 // items per workgroup of the prefix sums: 256 threads x 4

inline int64_t align16(int64_t bytes) { return (bytes + 15) & ~(int64_t)15; }

// ---------------------------------------------------------------------------------------------------------------------------- keys
// the cell of a coordinate, and whether the grid has it (grid_cell: the test is on the float)
__device__ __forceinline__ bool cell_of(float x, float origin, float cell, int64_t& c) { return grid_cell(cell_coord(x, origin, cell), c); }

// the moved row is stored whatever its key; the workgroup's flag word (cmr_scan_rows.h) goes to flag_counts_kernel<2, KEYS_FLAG_BITS, false>
__global__ __launch_bounds__(256) void map_keys_kernel(const float* __restrict__ pts, int64_t ld, int64_t N, const float* __restrict__ pose,
                                                       float ox, float oy, float oz, float cell, int64_t* __restrict__ keys,
                                                       float* __restrict__ moved, int32_t* __restrict__ part) {
  __shared__ int buf[256];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int flag = 0;
  if (i < N) {
    float T[12], qx, qy, qz;
    if (pose) pose_load(pose, T);
    int64_t key = KEY_DROPPED;
    if (scan_row(pts, ld, i, pose != nullptr, T, qx, qy, qz)) {
      int64_t cx, cy, cz;
      const bool ix = cell_of(qx, ox, cell, cx), iy = cell_of(qy, oy, cell, cy), iz = cell_of(qz, oz, cell, cz);
      key = ix && iy && iz ? pack_key(cx, cy, cz) : KEY_OUTSIDE;
    }
    keys[i] = key;
    moved[i * 3] = qx;
    moved[i * 3 + 1] = qy;
    moved[i * 3 + 2] = qz;
    flag = key == KEY_DROPPED ? row_flag<KEYS_FLAG_BITS>(ROW_DROPPED) : key == KEY_OUTSIDE ? row_flag<KEYS_FLAG_BITS>(ROW_OUTSIDE) : 0;
  }
  int total;
  scan256(flag, buf, total);
  if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// ---------------------------------------------------------------------------------------------------------------------------- plan
// The two sides of a merge and what the plan keeps of it in the workspace.  Item i of the MAP side is map row i (i < M), of the SCAN side
// scan voxel i (i < S); each side has one item more, i = M and i = S, which only carries the side's total in the prefix sums.
//   rank[i]  map side: the scan voxels with a smaller key;  scan side: the map rows with a smaller key (key_bound, lower)
//   hit      the other side holds the item's key, at rank[i]
//   keep     map side: the row's stamp after the insert -- `stamp` on a hit, its own otherwise -- is not below min_stamp
//            scan side: a miss, and `stamp` is not below min_stamp
//   ex[i]    the side's keeps before item i
// An item that is kept goes to output row  ex[i] + the other side's ex[rank[i]]:  the kept rows of both sides with a smaller key.
struct Side {
  const int64_t* __restrict__ keys;                               // the side's own keys, ascending and unique
  const int64_t* __restrict__ other;                              // the other side's
  const int32_t* __restrict__ stamps;                             // map side: the rows' stamps; scan side: null
  int64_t n, n_other;
  int32_t* __restrict__ rank;
  int32_t* __restrict__ ex;
  int32_t* __restrict__ tile;                                     // per tile of 1024 items: keeps | hits << 16, then the keeps before the tile
};
struct Plan {
  Side map, scan;
  int64_t tiles_map, tiles_scan;
  int32_t stamp, min_stamp;
};

__device__ __forceinline__ bool hit_at(const Side& s, int64_t i, int64_t rank) { return rank < s.n_other && s.other[rank] == s.keys[i]; }
__device__ __forceinline__ bool keep_of(const Side& s, int64_t i, bool hit, int32_t stamp, int32_t min_stamp) {
  return s.stamps ? (hit ? stamp : s.stamps[i]) >= min_stamp : !hit && stamp >= min_stamp;
}

// LOCATE: find rank[i], leave the tile's keeps and hits.  Otherwise: read rank[i] back, write ex[i] from the scanned tile totals.
template <bool LOCATE>
__global__ __launch_bounds__(256) void plan_kernel(Plan p) {
  __shared__ int buf[256];
  const bool scan_side = (int64_t)blockIdx.x >= p.tiles_map;
  const Side& s = scan_side ? p.scan : p.map;
  const int64_t tile = (int64_t)blockIdx.x - (scan_side ? p.tiles_map : 0);
  const int64_t base = tile * SCAN_TILE + threadIdx.x * 4;
  int f[4], c = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t i = base + u;
    f[u] = 0;
    if (i < s.n) {
      const int64_t rank = LOCATE ? key_bound(s.other, s.n_other, s.keys[i], false) : (int64_t)s.rank[i];
      if (LOCATE) s.rank[i] = (int32_t)rank;
      const bool hit = hit_at(s, i, rank);
      f[u] = (keep_of(s, i, hit, p.stamp, p.min_stamp) ? 1 : 0) | (hit ? 1 << 16 : 0);
    }
    c += f[u];
  }
  int total;
  const int before = scan256(c, buf, total);
  if (LOCATE) {
    if (threadIdx.x == 0) s.tile[tile] = total;
    return;
  }
  int64_t at = (int64_t)s.tile[tile] + (before & 0xFFFF);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t i = base + u;
    if (i <= s.n) s.ex[i] = (int32_t)at;
    at += f[u] & 0xFFFF;
  }
}

// one workgroup: the tile totals of both sides -> the keeps before every tile; sizes = rows of the new map, new, merged, removed
__global__ __launch_bounds__(256) void plan_scan_kernel(Plan p, int64_t* __restrict__ sizes) {
  __shared__ int buf[256];
  int64_t kept[2], hits = 0;
  for (int side = 0; side < 2; ++side) {
    const Side& s = side ? p.scan : p.map;
    const int64_t tiles = side ? p.tiles_scan : p.tiles_map;
    int64_t carry = 0;
    for (int64_t base = 0; base < tiles; base += 256) {
      const int64_t i = base + threadIdx.x;
      const int v = i < tiles ? s.tile[i] : 0;
      int total;
      const int excl = scan256(v & 0xFFFF, buf, total);
      if (i < tiles) s.tile[i] = (int32_t)(carry + excl);
      carry += total;
      if (side) {                                                 // every hit is seen from both sides; count the scan's
        int h;
        scan256(v >> 16, buf, h);
        hits += h;
      }
    }
    kept[side] = carry;
  }
  if (threadIdx.x != 0) return;
  const int64_t fresh = p.scan.n - hits, rows = kept[0] + kept[1];
  sizes[0] = rows;
  sizes[1] = fresh;
  sizes[2] = hits;
  sizes[3] = p.map.n + fresh - rows;
}

// --------------------------------------------------------------------------------------------------------------------------- write
struct Rows {
  const float* __restrict__ points;
  const float* __restrict__ attr;
  const int32_t* __restrict__ count;
};
// m' = ma + w (mb - ma), each operation rounded on its own
__device__ __forceinline__ float combine(float ma, float mb, float w) {
#pragma clang fp contract(off)
  const float d = mb - ma;
  const float wd = w * d;
  return ma + wd;
}

__global__ __launch_bounds__(256) void map_write_kernel(Plan p, Rows map, Rows scan, int C, int64_t* __restrict__ keys,
                                                        float* __restrict__ points, float* __restrict__ attr, int32_t* __restrict__ count,
                                                        int32_t* __restrict__ stamps) {
  const int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (item >= p.map.n + p.scan.n) return;
  const bool scan_side = item >= p.map.n;
  const Side& s = scan_side ? p.scan : p.map;
  const Side& other = scan_side ? p.map : p.scan;
  const int64_t i = item - (scan_side ? p.map.n : 0);
  const int64_t rank = s.rank[i];
  const bool hit = hit_at(s, i, rank);
  if (!keep_of(s, i, hit, p.stamp, p.min_stamp)) return;         // a hit is written from the map side
  const int64_t o = (int64_t)s.ex[i] + other.ex[rank];
  const Rows& own = scan_side ? scan : map;
  keys[o] = s.keys[i];
  if (!hit) {
#pragma unroll
    for (int c = 0; c < 3; ++c) points[o * 3 + c] = own.points[i * 3 + c];
    for (int c = 0; c < C; ++c) attr[o * C + c] = own.attr[i * C + c];
    count[o] = own.count[i];
    stamps[o] = scan_side ? p.stamp : s.stamps[i];
    return;
  }
  const int64_t ca = map.count[i], cb = scan.count[rank];
  const int64_t n = ca + cb < ROW_LIMIT - 1 ? ca + cb : ROW_LIMIT - 1;
  const float w = (float)cb / (float)n;
#pragma unroll
  for (int c = 0; c < 3; ++c) points[o * 3 + c] = combine(map.points[i * 3 + c], scan.points[rank * 3 + c], w);
  for (int c = 0; c < C; ++c) attr[o * C + c] = combine(map.attr[i * C + c], scan.attr[rank * C + c], w);
  count[o] = (int32_t)n;
  stamps[o] = p.stamp;
}

// the scan's voxel keys, one per run of the sorted rows
__global__ __launch_bounds__(256) void run_keys_kernel(const int64_t* __restrict__ keys_sorted, const int32_t* __restrict__ offsets, int64_t S,
                                                       int64_t* __restrict__ out) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s < S) out[s] = keys_sorted[offsets[s]];
}

// the workspace of a plan: the scan's keys, rank and ex of both sides, the tile totals of both sides
struct PlanSpace {
  int64_t scan_keys, rank_map, rank_scan, ex_map, ex_scan, tile_map, tile_scan, bytes, tiles_map, tiles_scan;
};
inline PlanSpace plan_space(int64_t M, int64_t S) {
  PlanSpace w;
  w.tiles_map = M / SCAN_TILE + 1;                                // M + 1 items: the last one carries the total
  w.tiles_scan = S / SCAN_TILE + 1;
  w.scan_keys = 0;
  w.rank_map = w.scan_keys + align16(S * 8);
  w.rank_scan = w.rank_map + align16(M * 4);
  w.ex_map = w.rank_scan + align16(S * 4);
  w.ex_scan = w.ex_map + align16((M + 1) * 4);
  w.tile_map = w.ex_scan + align16((S + 1) * 4);
  w.tile_scan = w.tile_map + align16(w.tiles_map * 4);
  w.bytes = w.tile_scan + align16(w.tiles_scan * 4);
  return w;
}
inline bool sizes_ok(int64_t M, int64_t S) { return M >= 0 && S >= 0 && M + S > 0 && M + S < ROW_LIMIT; }
inline Plan plan_of(const int64_t* map_keys, const int32_t* map_stamp, int64_t M, int64_t S, int stamp, int min_stamp, void* workspace) {
  const PlanSpace w = plan_space(M, S);
  char* ws = (char*)workspace;
  const int64_t* scan_keys = (const int64_t*)(ws + w.scan_keys);
  Plan p;
  p.map = Side{map_keys, scan_keys, map_stamp, M, S, (int32_t*)(ws + w.rank_map), (int32_t*)(ws + w.ex_map), (int32_t*)(ws + w.tile_map)};
  p.scan = Side{scan_keys, map_keys, nullptr, S, M, (int32_t*)(ws + w.rank_scan), (int32_t*)(ws + w.ex_scan), (int32_t*)(ws + w.tile_scan)};
  p.tiles_map = w.tiles_map;
  p.tiles_scan = w.tiles_scan;
  p.stamp = stamp;
  p.min_stamp = min_stamp;
  return p;
}

}  // namespace

extern "C" int64_t cmr_voxel_map_keys_workspace_bytes(int64_t N) { return N > 0 ? (N + 255) / 256 * 4 : 0; }

extern "C" int cmr_voxel_map_keys_f32(const float* points, int64_t ld, int64_t N, const float* pose, float ox, float oy, float oz, float voxel,
                                      int64_t* keys, float* moved, int64_t* counts, void* workspace, int64_t workspace_bytes,
                                      hipStream_t stream) {
  CMR_REQUIRE(points && keys && moved && counts && workspace && ld >= 3 && N > 0 && N < ROW_LIMIT && voxel > 0.f && isfinite(voxel) &&
              isfinite(ox) && isfinite(oy) && isfinite(oz) && workspace_bytes >= cmr_voxel_map_keys_workspace_bytes(N));
  const unsigned blocks = blocks_of(N, 256);
  hipLaunchKernelGGL(map_keys_kernel, dim3(blocks), dim3(256), 0, stream, points, ld, N, pose, ox, oy, oz, voxel, keys, moved,
                     (int32_t*)workspace);
  hipLaunchKernelGGL((flag_counts_kernel<2, KEYS_FLAG_BITS, false>), dim3(1), dim3(256), 0, stream, (const int32_t*)workspace, (int64_t)blocks, N,
                     counts);
  return cmr_launch_status();
}

extern "C" int64_t cmr_voxel_map_plan_workspace_bytes(int64_t M, int64_t S) { return sizes_ok(M, S) ? plan_space(M, S).bytes : 0; }

extern "C" int cmr_voxel_map_plan_i64(const int64_t* map_keys, const int32_t* map_stamp, int64_t M, const int64_t* keys_sorted,
                                      const int32_t* offsets, int64_t S, int stamp, int min_stamp, int64_t* sizes, void* workspace,
                                      int64_t workspace_bytes, hipStream_t stream) {
  CMR_REQUIRE(sizes_ok(M, S) && (M == 0 || (map_keys && map_stamp)) && (S == 0 || (keys_sorted && offsets)) && stamp >= 0 && min_stamp >= 0 &&
              sizes && workspace && cmr_aligned16(workspace) && workspace_bytes >= cmr_voxel_map_plan_workspace_bytes(M, S));
  const Plan p = plan_of(map_keys, map_stamp, M, S, stamp, min_stamp, workspace);
  const unsigned tiles = (unsigned)(p.tiles_map + p.tiles_scan);
  if (S > 0) hipLaunchKernelGGL(run_keys_kernel, dim3(blocks_of(S, 256)), dim3(256), 0, stream, keys_sorted, offsets, S, (int64_t*)workspace);
  hipLaunchKernelGGL(plan_kernel<true>, dim3(tiles), dim3(256), 0, stream, p);
  hipLaunchKernelGGL(plan_scan_kernel, dim3(1), dim3(256), 0, stream, p, sizes);
  hipLaunchKernelGGL(plan_kernel<false>, dim3(tiles), dim3(256), 0, stream, p);
  return cmr_launch_status();
}

extern "C" int cmr_voxel_map_write_f32(const int64_t* map_keys, const float* map_points, const float* map_attr, const int32_t* map_count,
                                       const int32_t* map_stamp, int64_t M, const float* scan_points, const float* scan_attr,
                                       const int32_t* scan_count, int64_t S, int C, int stamp, int min_stamp, const void* workspace,
                                       int64_t workspace_bytes, int64_t rows, int64_t* keys, float* points, float* attr, int32_t* count,
                                       int32_t* stamps, hipStream_t stream) {
  CMR_REQUIRE(sizes_ok(M, S) && C >= 0 && (M == 0 || (map_keys && map_points && map_count && map_stamp && (C == 0 || map_attr))) &&
              (S == 0 || (scan_points && scan_count && (C == 0 || scan_attr))) && stamp >= 0 && min_stamp >= 0 && workspace &&
              cmr_aligned16(workspace) && workspace_bytes >= cmr_voxel_map_plan_workspace_bytes(M, S) && rows >= 0 && rows <= M + S);
  if (rows == 0) return CMR_OK;
  CMR_REQUIRE(keys && points && count && stamps && (C == 0 || attr));
  const Plan p = plan_of(map_keys, map_stamp, M, S, stamp, min_stamp, const_cast<void*>(workspace));
  hipLaunchKernelGGL(map_write_kernel, dim3(blocks_of(M + S, 256)), dim3(256), 0, stream, p, Rows{map_points, map_attr, map_count},
                     Rows{scan_points, scan_attr, scan_count}, C, keys, points, attr, count, stamps);
  return cmr_launch_status();
}
