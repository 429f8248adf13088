// Point painting and z-buffered attribute rendering under a pose (port extension): the two directions between a cloud and
// an image once a pose is known.  Both project with cmr_project.h, the one statement of the fp32 fmaf chains and the in-view predicate
// that guided match, pose score and visibility use too, so "painted", "in view" (guided match at radius 0) and ops.visibility's cell are
// the same rows and cells bit for bit.
//
// cmr_paint_points_f32 -- the image laid over the cloud.  Two launches on the caller's stream:
//   cmr_zero_kernel   counts = 0 (cmr_common.h).
//   pi_paint_kernel   one thread per row on (ceil(N / 256), B): projection (pose and K are wave-uniform: scalar loads), the in-view test
//                     on the floats, then the C planes PI_PLANES at a time: the taps of all PI_PLANES planes (4 each when bilinear) are
//                     loaded before the first is used, the three lerps are rounded operation by operation (cmr_lerp, under
//                     fp contract(off): never an fma, so plain fp32 torch code gives the same bits), and colours are stored coalesced (consecutive
//                     n within a plane), 0 for the rows that are not painted.  counts by one atomic per workgroup and word.
// cmr_render_points_f32 -- the cloud laid over the image: a z-buffer that remembers its owner.  The key, its fill, its decode and the
// attribute gather are cmr_zbuffer.h's, shared with surfel.hip.  Three launches, no memset node:
//   pi_fill_kernel    key map = empty (cmr_zfill) and counts = 0.
//   pi_splat_kernel   one thread per row: a selected row in view lowers the key cmr_zkey(z, n) of its cell with ONE unsigned 64-bit vector
//                     atomic min: the map does not depend on the order of arrival.
//   pi_resolve_kernel one thread per pixel, templated on the footprint S = splat: the least key over the (2S + 1)^2 cells round the pixel as
//                     a gather -- compile-time loop bounds, clamped addresses and a select, all loads of a line in flight together; a
//                     minimum is exact, so this equals (2S + 1)^2 atomics per row -- then cmr_zresolve / cmr_zgather: coalesced stores of
//                     the index / depth / attribute maps.
// No floating-point atomic anywhere; every output element is a plain store by the thread that owns it.
#include "cmr_zbuffer.h"

namespace {

constexpr int PI_THREADS = 256;
constexpr int PI_PLANES = 4;       // planes whose taps are in flight together
constexpr int PI_MAX_SPLAT = 4;

template <bool BILINEAR>
__global__ __launch_bounds__(PI_THREADS) void pi_paint_kernel(const float* __restrict__ pts, const void* __restrict__ mask, int mask_bytes,
                                                              const float* __restrict__ pose, const float* __restrict__ Kin,
                                                              const float* __restrict__ image, int N, int C, int H, int W,
                                                              float* __restrict__ colors, uint8_t* __restrict__ painted,
                                                              int32_t* __restrict__ counts, float* __restrict__ uv) {
  __shared__ int part[2][PI_THREADS / 64];
  const int b = blockIdx.y, n = blockIdx.x * PI_THREADS + threadIdx.x;
  const int64_t g = (int64_t)b * N + n;
  const bool valid = n < N;
  const bool sel = valid && cmr_sel_or_all(mask, mask_bytes, g);
  CmrProj p;
  p.u = p.v = __builtin_nanf("");
  p.view = false;
  p.cx = p.cy = 0;
  if (sel) p = cmr_project(pose + 16 * b, Kin + 9 * b, pts + (int64_t)b * 3 * N, N, n, H, W, 0);
  const bool paint = sel && p.view;
  if (valid) {
    painted[g] = paint ? 1 : 0;
    if (uv) {
      uv[(int64_t)b * 2 * N + n] = p.u;
      uv[(int64_t)b * 2 * N + N + n] = p.v;
    }
  }
  // tap offsets inside a plane, all inside the image: an unpainted row reads nothing
  const CmrTaps tp = cmr_taps<BILINEAR>(p, paint, H, W);
  const int64_t plane = (int64_t)H * W;
  const float* img = image + (int64_t)b * C * plane;
  float* out = colors + (int64_t)b * C * N;
  for (int c = 0; c < C; c += PI_PLANES) {                               // wave-uniform
    float val[PI_PLANES];
#pragma unroll
    for (int k = 0; k < PI_PLANES; ++k) val[k] = 0.f;
    if (paint) {
      float t[PI_PLANES][4];
#pragma unroll
      for (int k = 0; k < PI_PLANES; ++k) {
        const float* ip = img + (int64_t)(c + k < C ? c + k : C - 1) * plane;
        t[k][0] = ip[tp.o00];
        if (BILINEAR) { t[k][1] = ip[tp.o01]; t[k][2] = ip[tp.o10]; t[k][3] = ip[tp.o11]; }
      }
#pragma unroll
      for (int k = 0; k < PI_PLANES; ++k)
        val[k] = cmr_tap_value<BILINEAR>(tp, t[k][0], t[k][1], t[k][2], t[k][3]);
    }
    if (valid) {
#pragma unroll
      for (int k = 0; k < PI_PLANES; ++k)
        if (c + k < C) out[(int64_t)(c + k) * N + n] = val[k];
    }
  }
  const bool flag[2] = {sel, paint};
  int cnt[2];
  cmr_block_counts<2, PI_THREADS>(flag, part, cnt);
  if (threadIdx.x < 2 && cnt[threadIdx.x]) atomicAdd(&counts[2 * b + threadIdx.x], cnt[threadIdx.x]);
}

__global__ __launch_bounds__(PI_THREADS) void pi_fill_kernel(unsigned long long* __restrict__ keys, int64_t cells,
                                                             int32_t* __restrict__ counts, int ncounts) {
  const int64_t i = (int64_t)blockIdx.x * PI_THREADS + threadIdx.x, stride = (int64_t)gridDim.x * PI_THREADS;
  cmr_zfill(keys, cells, i, stride);
  for (int64_t c = i; c < ncounts; c += stride) counts[c] = 0;
}

__global__ __launch_bounds__(PI_THREADS) void pi_splat_kernel(const float* __restrict__ pts, const void* __restrict__ mask, int mask_bytes,
                                                              const float* __restrict__ pose, const float* __restrict__ Kin, int N, int h,
                                                              int w, unsigned long long* __restrict__ keys, int32_t* __restrict__ counts) {
  __shared__ int part[2][PI_THREADS / 64];
  const int b = blockIdx.y, n = blockIdx.x * PI_THREADS + threadIdx.x;
  const bool sel = n < N && cmr_sel_or_all(mask, mask_bytes, (int64_t)b * N + n);
  bool view = false;
  if (sel) {
    const CmrProj p = cmr_project(pose + 16 * b, Kin + 9 * b, pts + (int64_t)b * 3 * N, N, n, h, w, 0);
    view = p.view;
    if (view) atomicMin(keys + (int64_t)b * h * w + (p.cy * w + p.cx), cmr_zkey(p.z, (unsigned)n));      // cy * w + cx < h * w <= 2^24
  }
  const bool flag[2] = {sel, view};
  int cnt[2];
  cmr_block_counts<2, PI_THREADS>(flag, part, cnt);
  if (threadIdx.x < 2 && cnt[threadIdx.x]) atomicAdd(&counts[3 * b + threadIdx.x], cnt[threadIdx.x]);
}

template <int S>
__global__ __launch_bounds__(PI_THREADS) void pi_resolve_kernel(const unsigned long long* __restrict__ keys, const float* __restrict__ attr,
                                                                int C, int N, int h, int w, float fill, int32_t* __restrict__ index_map,
                                                                float* __restrict__ depth_map, float* __restrict__ attr_map,
                                                                int32_t* __restrict__ counts) {
  __shared__ int part[1][PI_THREADS / 64];
  const int b = blockIdx.y, cells = h * w;
  const int i = blockIdx.x * PI_THREADS + threadIdx.x;
  const bool valid = i < cells;
  const int pix = valid ? i : cells - 1;
  const int py = pix / w, px = pix - py * w;
  const unsigned long long* kb = keys + (int64_t)b * cells;
  unsigned long long best = CMR_ZEMPTY;
#pragma unroll
  for (int dy = -S; dy <= S; ++dy) {
    const int y = py + dy;
    const bool iny = y >= 0 && y < h;
    const unsigned long long* line = kb + (int64_t)cmr_clampi(y, h - 1) * w;
    unsigned long long k[2 * S + 1];
#pragma unroll
    for (int dx = -S; dx <= S; ++dx) k[dx + S] = line[cmr_clampi(px + dx, w - 1)];
#pragma unroll
    for (int dx = -S; dx <= S; ++dx) {
      const int x = px + dx;
      const unsigned long long kk = (iny && x >= 0 && x < w) ? k[dx + S] : CMR_ZEMPTY;
      best = kk < best ? kk : best;
    }
  }
  const bool owned = cmr_zresolve(best, valid, b, i, cells, index_map, depth_map);
  cmr_zgather(best, owned, valid, b, i, cells, attr, C, N, fill, attr_map);
  const bool flag[1] = {owned};
  int cnt[1];
  cmr_block_counts<1, PI_THREADS>(flag, part, cnt);
  if (threadIdx.x == 0 && cnt[0]) atomicAdd(&counts[3 * b + 2], cnt[0]);
}

}  // namespace

extern "C" int cmr_paint_points_f32(const float* pts, const void* mask, int mask_bytes, const float* pose, const float* K, const float* image,
                                    int B, int N, int C, int H, int W, int mode, float* colors, uint8_t* painted, int32_t* counts, float* uv,
                                    hipStream_t stream) {
  CMR_REQUIRE(pts && pose && K && image && colors && painted && counts);
  CMR_REQUIRE(cmr_cloud_map_ok(B, N, H, W) && C >= 1 && C <= CMR_MAX_PLANES);
  CMR_REQUIRE(cmr_mask_bytes_ok(mask_bytes) && (mode == 0 || mode == 1));
  hipLaunchKernelGGL(cmr_zero_kernel<PI_THREADS>, dim3(1), dim3(PI_THREADS), 0, stream, counts, 2 * B);
  const dim3 grid((N + PI_THREADS - 1) / PI_THREADS, B);
  if (mode == 1)
    hipLaunchKernelGGL(pi_paint_kernel<true>, grid, dim3(PI_THREADS), 0, stream, pts, mask, mask_bytes, pose, K, image, N, C, H, W, colors,
                       painted, counts, uv);
  else
    hipLaunchKernelGGL(pi_paint_kernel<false>, grid, dim3(PI_THREADS), 0, stream, pts, mask, mask_bytes, pose, K, image, N, C, H, W, colors,
                       painted, counts, uv);
  return cmr_launch_status();
}

extern "C" int64_t cmr_render_points_workspace_bytes(int B, int h, int w) {
  return cmr_zkeys_bytes(B, h, w);
}

extern "C" int cmr_render_points_f32(const float* pts, const void* mask, int mask_bytes, const float* pose, const float* K, const float* attr,
                                     int C, int B, int N, int h, int w, int splat, float fill, int32_t* index_map, float* depth_map,
                                     float* attr_map, int32_t* counts, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  CMR_REQUIRE(pts && pose && K && index_map && depth_map && counts && workspace);
  CMR_REQUIRE(cmr_cloud_map_ok(B, N, h, w) && cmr_mask_bytes_ok(mask_bytes) && splat >= 0 && splat <= PI_MAX_SPLAT);
  CMR_REQUIRE(cmr_attr_ok(attr, attr_map, C));
  CMR_REQUIRE(cmr_aligned16(workspace) && workspace_bytes >= cmr_render_points_workspace_bytes(B, h, w));
  unsigned long long* keys = (unsigned long long*)workspace;
  const int64_t cells = (int64_t)B * h * w;
  const unsigned fill_blocks = cmr_fill_blocks(cells / 2, PI_THREADS);   // a 16-byte store per thread
  hipLaunchKernelGGL(pi_fill_kernel, dim3(fill_blocks), dim3(PI_THREADS), 0, stream, keys, cells, counts, 3 * B);
  hipLaunchKernelGGL(pi_splat_kernel, dim3((N + PI_THREADS - 1) / PI_THREADS, B), dim3(PI_THREADS), 0, stream, pts, mask, mask_bytes, pose, K,
                     N, h, w, keys, counts);
  const dim3 grid((h * w + PI_THREADS - 1) / PI_THREADS, B);
#define PI_RESOLVE(S)                                                                                                                  \
  case S:                                                                                                                              \
    hipLaunchKernelGGL(pi_resolve_kernel<S>, grid, dim3(PI_THREADS), 0, stream, (const unsigned long long*)keys, attr, C, N, h, w, fill, \
                       index_map, depth_map, attr_map, counts);                                                                        \
    break;
  switch (splat) {
    PI_RESOLVE(0)
    PI_RESOLVE(1)
    PI_RESOLVE(2)
    PI_RESOLVE(3)
    PI_RESOLVE(4)
  }
#undef PI_RESOLVE
  return cmr_launch_status();
}
