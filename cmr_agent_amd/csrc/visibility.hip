// Point visibility and depth rendering under a pose (port extension): a one-cell z-buffer of the occluder rows on the
// h x w map, then per queried row the test of its own depth against the nearest depth in the (2r + 1)^2 window round its centre.
//
// Three launches on the caller's stream, no memset node, whatever the data:
//   vis_fill_kernel   Z = +inf (16-byte stores on the aligned body, dwords on the head and tail) and counts = 0.
//   vis_splat_kernel  one thread per row: the rows of mask | occ_mask are projected (cmr_project.h, the predicate at radius 0) and their
//                     cell / depth written -- into the caller's arrays when given, else into the workspace; an occluder row in view
//                     lowers Z at its centre with an UNSIGNED INTEGER atomic min on the float's bits (positive floats order like their
//                     bit patterns; a vector atomic, order independent).  counts[3] by one atomic per workgroup.
//   vis_test_kernel   VT_LANES = 4 lanes per row, 64 rows per workgroup: the window is walked directly, a line at a time, lane j taking
//                     the columns cx - r + j, + 4, ...; VT_AHEAD loads are in flight together; the four partial minima meet over two
//                     quad-permute DPP moves.  Every loop bound is wave-uniform (all rows walk the whole square; a cell outside the map
//                     or past the line's end is read from the clamped address and replaced by +inf), so EXEC is full under the DPP
//                     moves; a wave without one selected row in view skips the walk.  bound = zmin * opr + abs_tol with the product
//                     and the sum rounded separately.  visible is stored by lane 0 of the row; counts[0..2] by one atomic per
//                     workgroup and word.
// Why the direct walk and not a separable min-pool of Z through LDS: at the shapes the op is used at (some 10^4 .. 10^5 queried rows,
// r <= 4) the walk reads rows * (2r + 1)^2 <= a few 10^6 cells that sit in L2, while a pool reads and writes the whole map twice
// (B h w up to 3.4 10^6 cells at 352 x 1216, B = 8) whatever the rows are and adds a launch.  DESIGN.md 4r has the counts.
#include "cmr_project.h"

namespace {

constexpr int VIS_THREADS = 256;
constexpr int VIS_MAX_RADIUS = 16;  // guided_match.hip GM_MAX_RADIUS
constexpr int VT_LANES = 4;         // lanes per row in the test: one DPP quad
constexpr int VT_ROWS = VIS_THREADS / VT_LANES;
constexpr int VT_AHEAD = 4;         // window cells whose loads are in flight together per lane

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
  __shared__ int part[3][VIS_THREADS / 64];
  const int b = blockIdx.y, n = blockIdx.x * VT_ROWS + (threadIdx.x >> 2), j = threadIdx.x & (VT_LANES - 1);
  const int64_t g = (int64_t)b * N + n;
  const bool valid = n < N;
  const bool sel = valid && cmr_sel(mask, mask_bytes, g);
  const int c = sel ? cell[g] : -1;
  const bool active = c >= 0;                                            // selected and in view
  const float z = active ? depth[g] : 0.f;
  const int cx = active ? c % w : 0, cy = active ? c / w : 0;
  const float* Zb = Z + (int64_t)b * h * w;
  const float inf = __builtin_huge_valf();
  float zmin = inf;
  if (__ballot(active)) {                                                // wave-uniform: EXEC stays full inside
    // the window as one run of (2r + 1) lines x nch steps of VT_LANES columns, VT_AHEAD steps per turn
    const int nch = (2 * radius + 1 + VT_LANES - 1) / VT_LANES, total = (2 * radius + 1) * nch;
    int dy = -radius, ch = 0;                                            // wave-uniform
    for (int k = 0; k < total; k += VT_AHEAD) {
      float f[VT_AHEAD];
      bool in[VT_AHEAD];
#pragma unroll
      for (int u = 0; u < VT_AHEAD; ++u) {
        const int dx = -radius + ch * VT_LANES + j;
        const int x = cx + dx, y = cy + dy;                              // past the end of the run dy = r + 1: dropped by k + u < total
        in[u] = k + u < total && dx <= radius && x >= 0 && x < w && y >= 0 && y < h;
        f[u] = Zb[(y < 0 ? 0 : (y >= h ? h - 1 : y)) * w + (x < 0 ? 0 : (x >= w ? w - 1 : x))];
        if (++ch == nch) { ch = 0; ++dy; }
      }
#pragma unroll
      for (int u = 0; u < VT_AHEAD; ++u) zmin = fminf(zmin, in[u] ? f[u] : inf);      // Z holds no NaN: +inf or a positive depth
    }
  }
  zmin = fminf(zmin, cmr_fdpp<0xB1>(zmin));                               // quad_perm:[1,0,3,2]; outside every branch
  zmin = fminf(zmin, cmr_fdpp<0x4E>(zmin));                               // quad_perm:[2,3,0,1]
  const float bound = cmr_mul_add_rn(zmin, opr, abs_tol);                // two roundings, never one fma
  const bool vis = active && z <= bound;
  const bool first = j == 0;
  if (valid && first) visible[g] = vis ? 1 : 0;
  const bool flag[3] = {sel && first, active && first, vis && first};
  int cnt[3];
  cmr_block_counts<3, VIS_THREADS>(flag, part, cnt);
  if (threadIdx.x < 3 && cnt[threadIdx.x]) atomicAdd(&counts[4 * b + threadIdx.x], cnt[threadIdx.x]);
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
  CMR_REQUIRE((mask_bytes == 1 || mask_bytes == 8) && (occ_mask_bytes == 1 || occ_mask_bytes == 8));
  CMR_REQUIRE(radius >= 0 && radius <= VIS_MAX_RADIUS);
  CMR_REQUIRE(rel_tol >= 0.f && abs_tol >= 0.f && __builtin_isfinite(rel_tol) && __builtin_isfinite(abs_tol));
  CMR_REQUIRE(cmr_aligned16(workspace) && workspace_bytes >= cmr_visibility_workspace_bytes(B, N, h, w));
  CMR_REQUIRE(!depth_map || (reinterpret_cast<uintptr_t>(depth_map) & 3u) == 0);
  const int64_t cells = (int64_t)B * h * w;
  char* ws = (char*)workspace;
  float* Z = depth_map ? depth_map : (float*)ws;
  int32_t* cellp = cell ? cell : (int32_t*)(ws + cmr_up16(cells * 4));
  float* depthp = depth ? depth : (float*)(ws + cmr_up16(cells * 4) + cmr_up16((int64_t)B * N * 4));
  const float opr = (float)(1.0 + (double)rel_tol);
  const unsigned fill_blocks = cmr_fill_blocks(cells / 4, VIS_THREADS);   // a float4 per thread
  hipLaunchKernelGGL(vis_fill_kernel, dim3(fill_blocks), dim3(VIS_THREADS), 0, stream, Z, cells, counts, 4 * B);
  hipLaunchKernelGGL(vis_splat_kernel, dim3((N + VIS_THREADS - 1) / VIS_THREADS, B), dim3(VIS_THREADS), 0, stream, pts, mask, mask_bytes,
                     occ_mask, occ_mask_bytes, pose, K, N, h, w, (unsigned*)Z, cellp, depthp, counts);
  hipLaunchKernelGGL(vis_test_kernel, dim3((N + VT_ROWS - 1) / VT_ROWS, B), dim3(VIS_THREADS), 0, stream, mask, mask_bytes, (const float*)Z,
                     (const int32_t*)cellp, (const float*)depthp, N, h, w, radius, opr, abs_tol, visible, counts);
  return cmr_launch_status();
}
