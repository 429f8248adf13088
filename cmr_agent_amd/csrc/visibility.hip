// Point visibility and depth rendering under a pose (port extension): a one-cell z-buffer of the occluder rows on the
// h x w map, then per queried row the test of its own depth against the nearest depth in the (2r + 1)^2 window round its centre.
//
// Three launches on the caller's stream, no memset node, whatever the data:
//   vis_fill_kernel   Z = +inf (16-byte stores on the aligned body, dwords on the head and tail) and counts = 0.
//   vis_splat_kernel  one thread per row: the rows of mask | occ_mask are projected (cmr_project.h, the predicate at radius 0) and their
//                     cell / depth written -- into the caller's arrays when given, else into the workspace; an occluder row in view
//                     lowers Z at its centre with an UNSIGNED INTEGER atomic min on the float's bits (positive floats order like their
//                     bit patterns; a vector atomic, order independent).  counts[3] by one atomic per workgroup.
//   vis_test_kernel   four lanes per row, 64 rows per workgroup: the stored cell and depth of a queried row, then cmr_ztest_row
//                     (cmr_zbuffer.h), the window walk, the bound, the store of visible and counts[0..2] that surfel.hip's depth test
//                     runs on a map the caller brings.
// Why the direct walk and not a separable min-pool of Z through LDS: at the shapes the op is used at (some 10^4 .. 10^5 queried rows,
// r <= 4) the walk reads rows * (2r + 1)^2 <= a few 10^6 cells that sit in L2, while a pool reads and writes the whole map twice
// (B h w up to 3.4 10^6 cells at 352 x 1216, B = 8) whatever the rows are and adds a launch.  DESIGN.md 4r has the counts.
#include "cmr_zbuffer.h"

namespace {

constexpr int VIS_THREADS = 256;
constexpr int VT_ROWS = VIS_THREADS / CMR_ZT_LANES;  // rows per workgroup in the test

__global__ __launch_bounds__(VIS_THREADS) void vis_fill_kernel(float* __restrict__ Z, int64_t total, int32_t* __restrict__ counts,
                                                               int ncounts) {
  const int64_t i = (int64_t)blockIdx.x * VIS_THREADS + threadIdx.x, stride = (int64_t)gridDim.x * VIS_THREADS;
  const float inf = __builtin_huge_valf();
  int64_t head = (int64_t)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(Z) & 15u)) & 15u) >> 2);
  head = head < total ? head : total;
  const int64_t nvec = (total - head) >> 2, tail = head + 4 * nvec;
  float4* Zv = reinterpret_cast<float4*>(Z + head);
  for (int64_t v = i; v < nvec; v += stride) Zv[v] = make_float4(inf, inf, inf, inf);
  if (i < head) Z[i] = inf;
  if (i < total - tail) Z[tail + i] = inf;
  for (int64_t c = i; c < ncounts; c += stride) counts[c] = 0;
}

__global__ __launch_bounds__(VIS_THREADS) void vis_splat_kernel(const float* __restrict__ pts, const void* __restrict__ mask, int mask_bytes,
                                                                const void* __restrict__ occ_mask, int occ_bytes,
                                                                const float* __restrict__ pose, const float* __restrict__ Kin, int N, int h,
                                                                int w, unsigned* __restrict__ Z, int32_t* __restrict__ cell,
                                                                float* __restrict__ depth, int32_t* __restrict__ counts) {
  __shared__ int part[1][VIS_THREADS / 64];
  const int b = blockIdx.y, n = blockIdx.x * VIS_THREADS + threadIdx.x;
  const int64_t g = (int64_t)b * N + n;
  const bool sel = n < N && cmr_sel(mask, mask_bytes, g);
  const bool occ = n < N && (occ_mask ? cmr_sel(occ_mask, occ_bytes, g) : true);
  bool view = false;
  int c = -1;
  float z = __builtin_nanf("");
  if (sel || occ) {
    const CmrProj p = cmr_project<true>(pose + 16 * b, Kin + 9 * b, pts + (int64_t)b * 3 * N, N, n, h, w, 0);
    z = p.z;
    view = p.view;
    c = p.cell;
  }
  if (n < N) {
    cell[g] = c;
    depth[g] = z;
  }
  if (occ && view) atomicMin(Z + (int64_t)b * h * w + c, __builtin_bit_cast(unsigned, z));
  const bool flag[1] = {occ && view};
  int nocc[1];
  cmr_block_counts<1, VIS_THREADS>(flag, part, nocc);
  if (threadIdx.x == 0 && nocc[0]) atomicAdd(&counts[4 * b + 3], nocc[0]);
}

__global__ __launch_bounds__(VIS_THREADS) void vis_test_kernel(const void* __restrict__ mask, int mask_bytes, const float* __restrict__ Z,
                                                               const int32_t* __restrict__ cell, const float* __restrict__ depth, int N,
                                                               int h, int w, int radius, float opr, float abs_tol,
                                                               uint8_t* __restrict__ visible, int32_t* __restrict__ counts) {
  const int b = blockIdx.y, n = blockIdx.x * VT_ROWS + (threadIdx.x >> 2);
  const int64_t g = (int64_t)b * N + n;
  const bool valid = n < N;
  const bool sel = valid && cmr_sel(mask, mask_bytes, g);
  const int c = sel ? cell[g] : -1;
  const float z = c >= 0 ? depth[g] : 0.f;
  cmr_ztest_row<VIS_THREADS, 4>(Z, b, h, w, radius, opr, abs_tol, valid, sel, c, z, g, visible, counts);
}

}  // namespace

extern "C" int64_t cmr_visibility_workspace_bytes(int B, int N, int h, int w) {
  if (B <= 0 || N <= 0 || h <= 0 || w <= 0) return 0;
  return cmr_up16((int64_t)B * h * w * 4) + 2 * cmr_up16((int64_t)B * N * 4);
}

extern "C" int cmr_visibility_f32(const float* pts, const void* mask, int mask_bytes, const void* occ_mask, int occ_mask_bytes,
                                  const float* pose, const float* K, int B, int N, int h, int w, int radius, float rel_tol, float abs_tol,
                                  uint8_t* visible, int32_t* counts, float* depth_map, int32_t* cell, float* depth, void* workspace,
                                  int64_t workspace_bytes, hipStream_t stream) {
  CMR_REQUIRE(pts && mask && pose && K && visible && counts && workspace);
  CMR_REQUIRE(cmr_cloud_map_ok(B, N, h, w));
  CMR_REQUIRE(cmr_mask_bytes_ok(mask_bytes) && cmr_mask_bytes_ok(occ_mask_bytes));
  CMR_REQUIRE(radius >= 0 && radius <= CMR_MAX_RADIUS);
  CMR_REQUIRE(cmr_tols_ok(rel_tol, abs_tol));
  CMR_REQUIRE(cmr_aligned16(workspace) && workspace_bytes >= cmr_visibility_workspace_bytes(B, N, h, w));
  CMR_REQUIRE(!depth_map || cmr_aligned4(depth_map));
  const int64_t cells = (int64_t)B * h * w;
  char* ws = (char*)workspace;
  float* Z = depth_map ? depth_map : (float*)ws;
  int32_t* cellp = cell ? cell : (int32_t*)(ws + cmr_up16(cells * 4));
  float* depthp = depth ? depth : (float*)(ws + cmr_up16(cells * 4) + cmr_up16((int64_t)B * N * 4));
  const float opr = cmr_one_plus(rel_tol);
  const unsigned fill_blocks = cmr_fill_blocks(cells / 4, VIS_THREADS);   // a float4 per thread
  hipLaunchKernelGGL(vis_fill_kernel, dim3(fill_blocks), dim3(VIS_THREADS), 0, stream, Z, cells, counts, 4 * B);
  hipLaunchKernelGGL(vis_splat_kernel, dim3((N + VIS_THREADS - 1) / VIS_THREADS, B), dim3(VIS_THREADS), 0, stream, pts, mask, mask_bytes,
                     occ_mask, occ_mask_bytes, pose, K, N, h, w, (unsigned*)Z, cellp, depthp, counts);
  hipLaunchKernelGGL(vis_test_kernel, dim3((N + VT_ROWS - 1) / VT_ROWS, B), dim3(VIS_THREADS), 0, stream, mask, mask_bytes, (const float*)Z,
                     (const int32_t*)cellp, (const float*)depthp, N, h, w, radius, opr, abs_tol, visible, counts);
  return cmr_launch_status();
}
