// Raw LiDAR scan -> the cloud files the loaders read: voxel-grid downsample and surface normals, one cloud per call.
//
//   cmr_cloud_bounds_f32     per-axis min / max over the rows with three finite coordinates, and their number
//   cmr_voxel_keys_f32       one int64 key per row from its grid cell (the contract of include/cmr_hip.h, bit for bit)
//   (the caller sorts the keys, stable: the rows of a cell become one run, in ascending input index)
//   cmr_segment_heads_i64    runs of equal keys -> CSR offsets, counts, the int32 row order cmr_segment_reduce_f32 takes, the inverse map
//   cmr_cloud_gather4_f32    the kept rows as float4 in key order: the rows of a grid index (ops.cloud_index; cloud_icp.hip searches them)
//   cmr_point_normals_f32    fixed-radius neighbourhoods over the sorted cells, 3x3 covariance, its smallest eigenvector
// The index, the walk over a neighbourhood's runs, the membership test and the workgroup scan live in cmr_cloud_grid.h (GridIndex, Walk, walk16, scan256), the Jacobi
// rotation and the finite test in cmr_common.h.
//
// No float atomics anywhere: min / max and the integer counts are order free, every float sum runs in a fixed order.
#include "cmr_cloud_grid.h"

namespace {

constexpr int64_t KEY_DROPPED = INT64_MAX;                      // rows with a non-finite coordinate sort behind every cell
constexpr int BOUNDS_BLOCKS = 256;                              // partial results of cmr_cloud_bounds_f32: 8 words each
constexpr int SCAN_TILE = 1024;                                 // rows per workgroup of the head scan: 256 threads x 4

// ------------------------------------------------------------------------------------------------------------------------ bounds
struct Bounds {
  float lo[3], hi[3];
  int kept;
};
__device__ __forceinline__ void bounds_merge(Bounds& a, const Bounds& b) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    a.lo[c] = fminf(a.lo[c], b.lo[c]);
    a.hi[c] = fmaxf(a.hi[c], b.hi[c]);
  }
  a.kept += b.kept;
}
// the workgroup's merged bounds in thread 0
__device__ __forceinline__ void bounds_block(Bounds& b, Bounds (&sh)[256]) {
  sh[threadIdx.x] = b;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) bounds_merge(sh[threadIdx.x], sh[threadIdx.x + off]);
    __syncthreads();
  }
  b = sh[0];
}
__device__ __forceinline__ void bounds_write(const Bounds& b, float* w) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    w[c] = b.lo[c];
    w[3 + c] = b.hi[c];
  }
  reinterpret_cast<int*>(w)[6] = b.kept;
}

__global__ __launch_bounds__(256) void bounds_partial_kernel(const float* __restrict__ pts, int64_t ld, int64_t N, float* __restrict__ part) {
  __shared__ Bounds sh[256];
  Bounds b{{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}, 0};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
    const float x = pts[i * ld], y = pts[i * ld + 1], z = pts[i * ld + 2];
    if (cmr_finite3(x, y, z)) bounds_merge(b, Bounds{{x, y, z}, {x, y, z}, 1});
  }
  bounds_block(b, sh);
  if (threadIdx.x == 0) bounds_write(b, part + (int64_t)blockIdx.x * 8);
}
__global__ __launch_bounds__(256) void bounds_final_kernel(const float* __restrict__ part, int blocks, float* __restrict__ bounds,
                                                           int64_t* __restrict__ kept) {
  __shared__ Bounds sh[256];
  Bounds b{{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}, 0};
  if ((int)threadIdx.x < blocks) {
    const float* w = part + threadIdx.x * 8;
    b = Bounds{{w[0], w[1], w[2]}, {w[3], w[4], w[5]}, reinterpret_cast<const int*>(w)[6]};
  }
  bounds_block(b, sh);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      bounds[c] = b.lo[c];
      bounds[3 + c] = b.hi[c];
    }
    kept[0] = b.kept;
  }
}

// -------------------------------------------------------------------------------------------------------------------------- keys
__global__ __launch_bounds__(256) void voxel_keys_kernel(const float* __restrict__ pts, int64_t ld, int64_t N, float ox, float oy, float oz,
                                                         float cell, int64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const float x = pts[i * ld], y = pts[i * ld + 1], z = pts[i * ld + 2];
  keys[i] = cmr_finite3(x, y, z) ? pack_key(cell_index(x, ox, cell), cell_index(y, oy, cell), cell_index(z, oz, cell)) : KEY_DROPPED;
}

// ------------------------------------------------------------------------------------------------------------------------- heads
// Row i of the sorted keys opens a run when it is the first row or its key differs from the row before it.  Three passes: heads per tile of
// 1024 rows, an exclusive scan of the tile totals by one workgroup, then every row's run number.
__device__ __forceinline__ int head_at(const int64_t* __restrict__ keys, int64_t i, int64_t kept) {
  return i < kept && (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
}
__global__ __launch_bounds__(256) void heads_count_kernel(const int64_t* __restrict__ keys, int64_t kept, int32_t* __restrict__ tile_sum) {
  __shared__ int buf[256];
  const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + threadIdx.x * 4;
  int c = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) c += head_at(keys, base + u, kept);
  int total;
  scan256(c, buf, total);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}
__global__ __launch_bounds__(256) void heads_scan_kernel(int32_t* __restrict__ tile_sum, int64_t tiles, int64_t* __restrict__ nseg) {
  __shared__ int buf[256];
  int64_t carry = 0;
  for (int64_t base = 0; base < tiles; base += 256) {
    const int64_t i = base + threadIdx.x;
    const int v = i < tiles ? tile_sum[i] : 0;
    int total;
    const int excl = scan256(v, buf, total);
    if (i < tiles) tile_sum[i] = (int32_t)(carry + excl);
    carry += total;
  }
  if (threadIdx.x == 0) nseg[0] = carry;
}
__global__ __launch_bounds__(256) void heads_write_kernel(const int64_t* __restrict__ keys, const int64_t* __restrict__ order, int64_t N,
                                                          int64_t kept, const int32_t* __restrict__ tile_sum, int64_t tiles,
                                                          int32_t* __restrict__ order32, int32_t* __restrict__ offsets,
                                                          int64_t* __restrict__ inverse) {
  __shared__ int buf[256];
  const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + threadIdx.x * 4;
  int f[4], c = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) c += f[u] = head_at(keys, base + u, kept);
  int total;
  int seg = scan256(c, buf, total) + ((int64_t)blockIdx.x < tiles ? tile_sum[blockIdx.x] : 0) - 1;       // run number of the row before `base`
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t i = base + u;
    if (i >= N) break;
    const int64_t row = order[i];
    if (i < kept) {
      seg += f[u];
      if (f[u]) offsets[seg] = (int32_t)i;
      if (i == kept - 1) offsets[seg + 1] = (int32_t)kept;
      order32[i] = (int32_t)row;
    }
    if (inverse) inverse[row] = i < kept ? seg : -1;
  }
}
__global__ __launch_bounds__(256) void heads_count_rows_kernel(const int32_t* __restrict__ offsets, const int64_t* __restrict__ nseg,
                                                               int32_t* __restrict__ count) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s < nseg[0]) count[s] = offsets[s + 1] - offsets[s];
}

// ----------------------------------------------------------------------------------------------------------------------- normals
__global__ __launch_bounds__(256) void gather_points4_kernel(const float* __restrict__ pts, int64_t ld, const int64_t* __restrict__ order,
                                                             int64_t kept, f32x4* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= kept) return;
  const float* p = pts + order[i] * ld;
  out[i] = f32x4{p[0], p[1], p[2], 0.f};
}

template <int I, int J>
__device__ __forceinline__ void eig_order(double (&w)[3], double (&v)[3][3]) {
  if (w[J] < w[I]) {
    const double t = w[I];
    w[I] = w[J];
    w[J] = t;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double u = v[k][I];
      v[k][I] = v[k][J];
      v[k][J] = u;
    }
  }
}

constexpr int JACOBI_SWEEPS = 8;      // cyclic Jacobi on a 3x3 in fp64 converges quadratically: five sweeps reach the last bit, eight are fixed

// One 16-lane group per query, in key order: the four queries of a wave are neighbours in space and read nearly the same runs.  The walk over
// the runs of the cells round the query is walk16 (cmr_cloud_grid.h); the grid's cell is the radius here.
__global__ __launch_bounds__(256) void point_normals_kernel(GridIndex index, int64_t N, float vx, float vy, float vz, int kmin,
                                                            float* __restrict__ normals, int32_t* __restrict__ count,
                                                            float* __restrict__ eig) {
  const int lane = threadIdx.x & 15;
  const int64_t q = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const bool live = q < index.kept;
  const f32x4 p = index.pts4[live ? q : 0];
  const Walk walk(p, live, index);
  const float r2 = index.cell * index.cell;

  float s[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // sum d (3), sum d d^T (xx xy xz yy yz zz)
  int k = 0;
  walk16(index, walk, lane, [&](int64_t, const f32x4& c) {
    const float dx = c.x - p.x, dy = c.y - p.y, dz = c.z - p.z;
    if (within(dx, dy, dz, r2)) {
      s[0] += dx;
      s[1] += dy;
      s[2] += dz;
      s[3] += dx * dx;
      s[4] += dx * dy;
      s[5] += dx * dz;
      s[6] += dy * dy;
      s[7] += dy * dz;
      s[8] += dz * dz;
      ++k;
    }
  });
  // every lane of the wave is here again: the lane sums in the fixed order of the DPP butterfly, pinned in front of the branches below
#pragma unroll
  for (int c = 0; c < 9; ++c) {
    s[c] = cmr_sum16(s[c]);
    asm volatile("" : "+v"(s[c]));
  }
  k = isum16(k);
  asm volatile("" : "+v"(k));

  const bool valid = live && k >= kmin;
  double w[3] = {0.0, 0.0, 0.0};
  double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  if (valid) {
    // C = sum d d^T / k - m m^T from the fp32 sums, in fp64
    const double inv = 1.0 / (double)k;
    const double mx = s[0] * inv, my = s[1] * inv, mz = s[2] * inv;
    double a[3][3];
    a[0][0] = s[3] * inv - mx * mx;
    a[0][1] = a[1][0] = s[4] * inv - mx * my;
    a[0][2] = a[2][0] = s[5] * inv - mx * mz;
    a[1][1] = s[6] * inv - my * my;
    a[1][2] = a[2][1] = s[7] * inv - my * mz;
    a[2][2] = s[8] * inv - mz * mz;
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
      cmr_jacobi_rotate<0, 1>(a, v);
      cmr_jacobi_rotate<0, 2>(a, v);
      cmr_jacobi_rotate<1, 2>(a, v);
    }
    w[0] = a[0][0];
    w[1] = a[1][1];
    w[2] = a[2][2];
    eig_order<0, 1>(w, v);
    eig_order<1, 2>(w, v);
    eig_order<0, 1>(w, v);
  }
  if (lane != 0 || q >= N) return;
  const int64_t row = index.order[q];
  float n[3] = {0.f, 0.f, 0.f};
  if (valid) {
    double nx = v[0][0], nyv = v[1][0], nz = v[2][0];
    const double len = sqrt(nx * nx + nyv * nyv + nz * nz);
    const double towards = nx * ((double)vx - p.x) + nyv * ((double)vy - p.y) + nz * ((double)vz - p.z);
    const double sc = (towards < 0.0 ? -1.0 : 1.0) / len;
    n[0] = (float)(nx * sc);
    n[1] = (float)(nyv * sc);
    n[2] = (float)(nz * sc);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    normals[row * 3 + c] = n[c];
    if (eig) eig[row * 3 + c] = (float)w[c];
  }
  count[row] = live ? k : 0;
}

}  // namespace

extern "C" int64_t cmr_cloud_bounds_workspace_bytes(int64_t N) { return N > 0 ? (int64_t)BOUNDS_BLOCKS * 8 * 4 : 0; }

extern "C" int cmr_cloud_bounds_f32(const float* points, int64_t ld, int64_t N, float* bounds, int64_t* kept, void* workspace,
                                    int64_t workspace_bytes, hipStream_t stream) {
  CMR_REQUIRE(points && bounds && kept && workspace && ld >= 3 && N > 0 && N < ((int64_t)1 << 31) &&
              workspace_bytes >= cmr_cloud_bounds_workspace_bytes(N));
  const int64_t want = (N + 255) / 256;
  const int blocks = (int)(want < BOUNDS_BLOCKS ? want : BOUNDS_BLOCKS);
  hipLaunchKernelGGL(bounds_partial_kernel, dim3(blocks), dim3(256), 0, stream, points, ld, N, (float*)workspace);
  hipLaunchKernelGGL(bounds_final_kernel, dim3(1), dim3(256), 0, stream, (const float*)workspace, blocks, bounds, kept);
  return cmr_launch_status();
}

extern "C" int cmr_voxel_keys_f32(const float* points, int64_t ld, int64_t N, float ox, float oy, float oz, float cell, int64_t* keys,
                                  hipStream_t stream) {
  CMR_REQUIRE(points && keys && ld >= 3 && N > 0 && N < ((int64_t)1 << 31) && cell > 0.f && isfinite(cell) && isfinite(ox) && isfinite(oy) &&
              isfinite(oz));
  hipLaunchKernelGGL(voxel_keys_kernel, dim3(blocks_of(N, 256)), dim3(256), 0, stream, points, ld, N, ox, oy, oz, cell, keys);
  return cmr_launch_status();
}

extern "C" int64_t cmr_segment_heads_workspace_bytes(int64_t N) { return N > 0 ? (N + SCAN_TILE - 1) / SCAN_TILE * 4 : 0; }

extern "C" int cmr_segment_heads_i64(const int64_t* keys_sorted, const int64_t* order, int64_t N, int64_t kept, int32_t* order32,
                                     int32_t* offsets, int32_t* count, int64_t* inverse, int64_t* nseg, void* workspace,
                                     int64_t workspace_bytes, hipStream_t stream) {
  CMR_REQUIRE(keys_sorted && order && order32 && offsets && count && nseg && workspace && N > 0 && N < ((int64_t)1 << 31) && kept > 0 &&
              kept <= N && workspace_bytes >= cmr_segment_heads_workspace_bytes(N));
  const int64_t tiles = (kept + SCAN_TILE - 1) / SCAN_TILE;
  int32_t* tile_sum = (int32_t*)workspace;
  hipLaunchKernelGGL(heads_count_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, keys_sorted, kept, tile_sum);
  hipLaunchKernelGGL(heads_scan_kernel, dim3(1), dim3(256), 0, stream, tile_sum, tiles, nseg);
  hipLaunchKernelGGL(heads_write_kernel, dim3(blocks_of(inverse ? N : kept, SCAN_TILE)), dim3(256), 0, stream, keys_sorted, order,
                     inverse ? N : kept, kept, tile_sum, tiles, order32, offsets, inverse);
  hipLaunchKernelGGL(heads_count_rows_kernel, dim3(blocks_of(kept, 256)), dim3(256), 0, stream, offsets, nseg, count);
  return cmr_launch_status();
}

extern "C" int cmr_cloud_gather4_f32(const float* points, int64_t ld, const int64_t* order, int64_t kept, float* points4, hipStream_t stream) {
  CMR_REQUIRE(points && order && points4 && ld >= 3 && kept > 0 && kept < ((int64_t)1 << 31) && cmr_aligned16(points4));
  hipLaunchKernelGGL(gather_points4_kernel, dim3(blocks_of(kept, 256)), dim3(256), 0, stream, points, ld, order, kept, (f32x4*)points4);
  return cmr_launch_status();
}

extern "C" int cmr_point_normals_f32(const float* points, int64_t ld, const int64_t* keys_sorted, const int64_t* order, int64_t N,
                                     int64_t kept, float ox, float oy, float oz, float radius, float vx, float vy, float vz,
                                     int min_neighbors, float* points4, float* normals, int32_t* count, float* eigenvalues,
                                     hipStream_t stream) {
  const GridIndex index{(const f32x4*)points4, keys_sorted, order, kept, ox, oy, oz, radius};      // the keys were taken with the radius as the cell
  CMR_REQUIRE(points && normals && count && ld >= 3 && N > 0 && N < ((int64_t)1 << 31) && grid_index_ok(index) && kept <= N && isfinite(vx) &&
              isfinite(vy) && isfinite(vz));
  hipLaunchKernelGGL(gather_points4_kernel, dim3(blocks_of(kept, 256)), dim3(256), 0, stream, points, ld, order, kept, (f32x4*)points4);
  hipLaunchKernelGGL(point_normals_kernel, dim3(blocks_of(N, 16)), dim3(256), 0, stream, index, N, vx, vy, vz,
                     min_neighbors < 3 ? 3 : min_neighbors, normals, count, eigenvalues);
  return cmr_launch_status();
}
