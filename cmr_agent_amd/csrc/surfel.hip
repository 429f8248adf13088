// Oriented-disc (surfel) rendering of the cloud from its normals, and the depth test against a map the caller brings (port extension,
// DESIGN.md 4z).  Every selected point is a disc in space -- centred on the point, perpendicular to its normal, r = radius +
// range_slope z_c metres -- and every pixel of its window intersects its own ray with that disc's plane.  The projection is
// cmr_project.h's (so the centre's cell and "in view" agree bit for bit with guided match, visibility, paint and render); the per-pixel
// part is plain fp32 operators under fp contract(off), each rounded on its own, so a numpy float32 restatement gives the same bits.
//
// cmr_render_surfels_f32 -- three launches on the caller's stream, no memset node, whatever the data.  The key, its fill, its decode and
// the attribute gather are cmr_zbuffer.h's, shared with point_image.hip:
//   sf_fill_kernel     key map = empty (cmr_zfill), counts[b] = (0, 0, 0, status of K[b]).
//   sf_splat_kernel    256 rows per workgroup in two phases.  Setup, one thread per row (coalesced loads, pose and K wave-uniform): the
//                      projection, X_c, n_c, r, the drawn predicate and the window the row walks, left in LDS (11 words per row); the
//                      `surfel` planes are stored here, coalesced; counts (selected, drawn) by one atomic per workgroup and word.
//                      Walk, one 16-lane group per row (16 groups, 16 rows each in turn): the window a line at a time, the lanes over the
//                      columns, so a wide footprint and a narrow one keep 16 lanes busy alike.  A covered pixel lowers the key
//                      cmr_zkey(tau, n) of its cell with ONE unsigned 64-bit vector atomic min -- after an L2-served load
//                      of the cell that skips the atomic when the stored key is already lower (keys only fall, so a stale value costs an
//                      atomic and never a result).  Why the skip: an atomic drops the line from the XCD's L2 and is one request per
//                      lane at the memory side; where discs overlap (a wall seen by several rings) most candidates lose, and the load
//                      keeps the line.  Not measured against unconditional atomics.
//   sf_resolve_kernel  one thread per pixel: cmr_zresolve (index / depth maps), then the owner's normal, recomputed from pts and normals
//                      (two gathers of three) for normal_map, then cmr_zgather (attribute map).  counts[2] by one atomic per workgroup.
// cmr_depth_test_f32 -- two launches: cmr_zero_kernel (counts = 0, cmr_common.h) and sf_test_kernel: the projection, then cmr_ztest_row,
//   the test visibility.hip runs on the cell and depth it stored.
// No floating-point atomic anywhere; every output element is a plain store by the thread that owns it.  No scratch.
#include "cmr_zbuffer.h"

namespace {

constexpr int SF_THREADS = 256;
constexpr int SF_LANES = 16;                       // lanes per surfel in the walk
constexpr int SF_GROUPS = SF_THREADS / SF_LANES;   // surfels walked together per workgroup
constexpr int SFT_ROWS = SF_THREADS / CMR_ZT_LANES; // rows per workgroup in the depth test

// The camera model the per-pixel part assumes: K = [[fx, s, cx], [0, fy, cy], [0, 0, 1]] with fx, fy finite and > 0.
__device__ __forceinline__ bool sf_camera_ok(const float* K) {
  return K[3] == 0.f && K[6] == 0.f && K[7] == 0.f && K[8] == 1.f && isfinite(K[0]) && K[0] > 0.f && isfinite(K[4]) && K[4] > 0.f;
}

// Row constants of the per-pixel part, each operation rounded on its own.
struct SfDisc {
  float xc, yc, zc, nx, ny, nz;
  float n2, nX, r2, g2;        // (nx^2 + ny^2) + nz^2; (nx xc + ny yc) + nz zc; r r; (min_cos min_cos) n2
};
__device__ __forceinline__ void sf_disc_constants(SfDisc& d, float r, float min_cos) {
#pragma clang fp contract(off)
  d.n2 = (d.nx * d.nx + d.ny * d.ny) + d.nz * d.nz;
  d.nX = (d.nx * d.xc + d.ny * d.yc) + d.nz * d.zc;
  d.r2 = r * r;
  d.g2 = (min_cos * min_cos) * d.n2;
}

// The ray of pixel (xf, yf) against the disc: covered or not, and its depth tau.  include/cmr_hip.h states these operations one by one.
__device__ __forceinline__ bool sf_ray(const SfDisc& d, float fx, float s, float cx, float fy, float cy, float xf, float yf, float& tau) {
#pragma clang fp contract(off)
  const float dy = (yf - cy) / fy;
  const float dx = ((xf - cx) - s * dy) / fx;
  bool ok = true;
  float oz = 0.f;
  if (d.n2 == 0.f) {
    tau = d.zc;
  } else {
    const float nd = (d.nx * dx + d.ny * dy) + d.nz;
    tau = d.nX / nd;
    ok = nd != 0.f && isfinite(tau) && tau > 0.f;
    const float q = (dx * dx + dy * dy) + 1.f;
    ok = ok && nd * nd >= d.g2 * q;
    oz = tau - d.zc;
  }
  const float ox = tau * dx - d.xc, oy = tau * dy - d.yc;
  return ok && (ox * ox + oy * oy) + oz * oz <= d.r2;
}

__global__ __launch_bounds__(SF_THREADS) void sf_fill_kernel(unsigned long long* __restrict__ keys, int64_t cells,
                                                             const float* __restrict__ Kin, int B, int32_t* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * SF_THREADS + threadIdx.x, stride = (int64_t)gridDim.x * SF_THREADS;
  cmr_zfill(keys, cells, i, stride);
  for (int64_t c = i; c < 4 * (int64_t)B; c += stride) counts[c] = (c & 3) == 3 ? (sf_camera_ok(Kin + 9 * (c >> 2)) ? 0 : 1) : 0;
}

__global__ __launch_bounds__(SF_THREADS) void sf_splat_kernel(const float* __restrict__ pts, const float* __restrict__ normals,
                                                              const void* __restrict__ mask, int mask_bytes,
                                                              const float* __restrict__ pose, const float* __restrict__ Kin, int N, int h,
                                                              int w, float radius, float range_slope, int max_px, float min_cos,
                                                              unsigned long long* __restrict__ keys, int32_t* __restrict__ counts,
                                                              float* __restrict__ surfel) {
  __shared__ int part[2][SF_THREADS / 64];
  __shared__ float rowf[7][SF_THREADS];            // xc yc zc ncx ncy ncz r
  __shared__ int roww[4][SF_THREADS];              // x0 x1 y0 y1, inclusive and inside the map; y1 < y0: nothing to walk
  const int b = blockIdx.y, t = threadIdx.x;
  const int64_t n = (int64_t)blockIdx.x * SF_THREADS + t;
  const float* P = pose + 16 * b;
  const float* K = Kin + 9 * b;
  const bool cam = sf_camera_ok(K);                                      // wave-uniform
  const float fx = K[0], s = K[1], cx = K[2], fy = K[4], cy = K[5];
  const bool valid = n < N;
  const bool sel = valid && cmr_sel_or_all(mask, mask_bytes, (int64_t)b * N + n);
  const float nan = __builtin_nanf("");
  float v[7] = {nan, nan, nan, nan, nan, nan, nan};
  int x0 = 0, x1 = -1, y0 = 0, y1 = -1;
  bool drawn = false;
  if (sel && cam) {
    const float* x = pts + (int64_t)b * 3 * N;
    const float* nr = normals + (int64_t)b * 3 * N;
    const CmrProj p = cmr_project(P, K, x, N, (int)n, h, w, max_px);
    const float a0 = nr[n], a1 = nr[N + n], a2 = nr[2 * (int64_t)N + n];
    float xc, yc, zc, ncx, ncy, ncz;
    cmr_camera_chains(P, x[n], x[N + n], x[2 * (int64_t)N + n], xc, yc, zc);
    cmr_rotate_chains(P, a0, a1, a2, ncx, ncy, ncz);
    const float r = cmr_mul_add_rn(range_slope, zc, radius);
    drawn = p.view && isfinite(a0) && isfinite(a1) && isfinite(a2) && isfinite(r) && r > 0.f && zc > r;
    if (drawn) {
      v[0] = xc; v[1] = yc; v[2] = zc; v[3] = ncx; v[4] = ncy; v[5] = ncz; v[6] = r;
      // The window walked.  A covered pixel's ray meets the disc at Q = X_c + o with |o| <= r, so Q_z >= z_c - r > 0 and
      //   Q_y / Q_z - y_c / z_c = (o_y - (y_c / z_c) o_z) / Q_z,  at most  r sqrt(1 + (y_c / z_c)^2) / (z_c - r)  in size,
      // likewise in x; with u - c_x = f_x X/Z + s Y/Z the pixel lies within
      //   hx = (f_x (1 + |x_c / z_c|) + |s| (1 + |y_c / z_c|)) r / (z_c - r),   hy = f_y (1 + |y_c / z_c|) r / (z_c - r)
      // of the centre (u, v) (sqrt(1 + a^2) <= 1 + |a|).  Rounding moves the fp32 rim by far less than a pixel, so the bound is
      // widened by 2^-12 of itself and one pixel, and the window is its intersection with the (2 max_px + 1)^2 window and the map.
      const float g = r / (zc - r), ax = 1.f + fabsf(xc / zc), ay = 1.f + fabsf(yc / zc), mp = (float)max_px;
      const float hx = fminf(((fx * ax + fabsf(s) * ay) * g) * 1.000244140625f + 1.f, mp + 1.f);     // fminf drops a NaN
      const float hy = fminf(((fy * ay) * g) * 1.000244140625f + 1.f, mp + 1.f);
      const int lx = (int)floorf(p.u - hx), ux = (int)ceilf(p.u + hx), ly = (int)floorf(p.v - hy), uy = (int)ceilf(p.v + hy);
      x0 = max(max(p.cx - max_px, lx), 0);
      x1 = min(min(p.cx + max_px, ux), w - 1);
      y0 = max(max(p.cy - max_px, ly), 0);
      y1 = min(min(p.cy + max_px, uy), h - 1);
      if (x1 < x0) y1 = y0 - 1;
    }
  }
#pragma unroll
  for (int k = 0; k < 7; ++k) rowf[k][t] = v[k];
  roww[0][t] = x0; roww[1][t] = x1; roww[2][t] = y0; roww[3][t] = y1;
  if (surfel && valid) {
    float* so = surfel + (int64_t)b * 8 * N + n;
#pragma unroll
    for (int k = 0; k < 7; ++k) so[(int64_t)k * N] = v[k];
    so[(int64_t)7 * N] = drawn ? 1.f : 0.f;
  }
  const bool flag[2] = {sel, drawn};
  int cnt[2];
  cmr_block_counts<2, SF_THREADS>(flag, part, cnt);                      // holds the barrier the walk needs
  if (t < 2 && cnt[t]) atomicAdd(&counts[4 * b + t], cnt[t]);
  if (cnt[1] == 0) return;                                               // workgroup-uniform

  const int grp = t / SF_LANES, j = t % SF_LANES;
  unsigned long long* kb = keys + (int64_t)b * h * w;
  for (int it = 0; it < SF_THREADS / SF_GROUPS; ++it) {
    const int i = it * SF_GROUPS + grp;
    const int wy0 = roww[2][i], wy1 = roww[3][i];
    if (wy1 < wy0) continue;                                             // uniform over the group
    const int wx0 = roww[0][i], wx1 = roww[1][i];
    SfDisc d;
    d.xc = rowf[0][i]; d.yc = rowf[1][i]; d.zc = rowf[2][i]; d.nx = rowf[3][i]; d.ny = rowf[4][i]; d.nz = rowf[5][i];
    sf_disc_constants(d, rowf[6][i], min_cos);
    const unsigned row = (unsigned)(blockIdx.x * SF_THREADS + i);
    for (int y = wy0; y <= wy1; ++y) {
      for (int x = wx0 + j; x <= wx1; x += SF_LANES) {
        float tau;
        if (sf_ray(d, fx, s, cx, fy, cy, (float)x, (float)y, tau)) {
          const unsigned long long key = cmr_zkey(tau, row);
          unsigned long long* cell = kb + (y * w + x);                   // y * w + x < h * w <= 2^24
          if (__hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key) atomicMin(cell, key);
        }
      }
    }
  }
}

__global__ __launch_bounds__(SF_THREADS) void sf_resolve_kernel(const unsigned long long* __restrict__ keys, const float* __restrict__ pts,
                                                                const float* __restrict__ normals, const float* __restrict__ pose,
                                                                const float* __restrict__ attr, int C, int N, int h, int w, float fill,
                                                                int32_t* __restrict__ index_map, float* __restrict__ depth_map,
                                                                float* __restrict__ normal_map, float* __restrict__ attr_map,
                                                                int32_t* __restrict__ counts) {
  __shared__ int part[1][SF_THREADS / 64];
  const int b = blockIdx.y, cells = h * w;
  const int i = blockIdx.x * SF_THREADS + threadIdx.x;
  const bool valid = i < cells;
  const unsigned long long best = keys[(int64_t)b * cells + (valid ? i : cells - 1)];
  const bool owned = cmr_zresolve(best, valid, b, i, cells, index_map, depth_map);
  if (normal_map) {
    float m0 = 0.f, m1 = 0.f, m2 = 0.f;
    if (owned) {
      const int owner = cmr_zowner(best);
      const float* x = pts + (int64_t)b * 3 * N;
      const float* nr = normals + (int64_t)b * 3 * N;
      const float* P = pose + 16 * b;
      SfDisc d;
      cmr_camera_chains(P, x[owner], x[N + owner], x[2 * (int64_t)N + owner], d.xc, d.yc, d.zc);
      cmr_rotate_chains(P, nr[owner], nr[N + owner], nr[2 * (int64_t)N + owner], d.nx, d.ny, d.nz);
      sf_disc_constants(d, 0.f, 0.f);
      if (d.n2 == 0.f) {
        m2 = -1.f;
      } else {
#pragma clang fp contract(off)
        const float len = sqrtf(d.n2);
        m0 = d.nx / len; m1 = d.ny / len; m2 = d.nz / len;
        if (d.nX > 0.f) { m0 = -m0; m1 = -m1; m2 = -m2; }                // n . X_c > 0 looks away from the camera: turn it
      }
    }
    if (valid) {
      float* nm = normal_map + (int64_t)b * 3 * cells + i;
      nm[0] = m0; nm[cells] = m1; nm[2 * (int64_t)cells] = m2;
    }
  }
  cmr_zgather(best, owned, valid, b, i, cells, attr, C, N, fill, attr_map);
  const bool flag[1] = {owned};
  int cnt[1];
  cmr_block_counts<1, SF_THREADS>(flag, part, cnt);
  if (threadIdx.x == 0 && cnt[0]) atomicAdd(&counts[4 * b + 2], cnt[0]);
}

__global__ __launch_bounds__(SF_THREADS) void sf_test_kernel(const float* __restrict__ pts, const void* __restrict__ mask, int mask_bytes,
                                                             const float* __restrict__ pose, const float* __restrict__ Kin,
                                                             const float* __restrict__ Z, int N, int h, int w, int radius, float opr,
                                                             float abs_tol, uint8_t* __restrict__ visible, int32_t* __restrict__ counts) {
  const int b = blockIdx.y;
  const int64_t n = (int64_t)blockIdx.x * SFT_ROWS + (threadIdx.x >> 2);
  const int64_t g = (int64_t)b * N + n;
  const bool valid = n < N;
  const bool sel = valid && cmr_sel(mask, mask_bytes, g);
  int c = -1;
  float z = 0.f;
  if (sel) {
    const CmrProj p = cmr_project<true>(pose + 16 * b, Kin + 9 * b, pts + (int64_t)b * 3 * N, N, (int)n, h, w, 0);
    c = p.cell;
    z = p.z;
  }
  cmr_ztest_row<SF_THREADS, 3>(Z, b, h, w, radius, opr, abs_tol, valid, sel, c, z, g, visible, counts);
}

}  // namespace

extern "C" int64_t cmr_render_surfels_workspace_bytes(int B, int h, int w) {
  return cmr_zkeys_bytes(B, h, w);
}

extern "C" int cmr_render_surfels_f32(const float* pts, const float* normals, const void* mask, int mask_bytes, const float* pose,
                                      const float* K, const float* attr, int C, int B, int N, int h, int w, float radius, float range_slope,
                                      int max_px, float min_cos, float fill, int32_t* index_map, float* depth_map, float* normal_map,
                                      float* attr_map, int32_t* counts, float* surfel, void* workspace, int64_t workspace_bytes,
                                      hipStream_t stream) {
  CMR_REQUIRE(pts && normals && pose && K && index_map && depth_map && counts && workspace);
  CMR_REQUIRE(cmr_cloud_map_ok(B, N, h, w) && cmr_mask_bytes_ok(mask_bytes) && max_px >= 0 && max_px <= CMR_MAX_RADIUS);
  CMR_REQUIRE(__builtin_isfinite(radius) && radius >= 0.f && __builtin_isfinite(range_slope) && range_slope >= 0.f);
  CMR_REQUIRE(min_cos >= 0.f && min_cos <= 1.f);
  CMR_REQUIRE(cmr_attr_ok(attr, attr_map, C));
  CMR_REQUIRE(cmr_aligned16(workspace) && workspace_bytes >= cmr_render_surfels_workspace_bytes(B, h, w));
  unsigned long long* keys = (unsigned long long*)workspace;
  const int64_t cells = (int64_t)B * h * w;
  const unsigned fill_blocks = cmr_fill_blocks(cells / 2, SF_THREADS);   // a 16-byte store per thread
  hipLaunchKernelGGL(sf_fill_kernel, dim3(fill_blocks), dim3(SF_THREADS), 0, stream, keys, cells, K, B, counts);
  hipLaunchKernelGGL(sf_splat_kernel, dim3((N + SF_THREADS - 1) / SF_THREADS, B), dim3(SF_THREADS), 0, stream, pts, normals, mask, mask_bytes,
                     pose, K, N, h, w, radius, range_slope, max_px, min_cos, keys, counts, surfel);
  hipLaunchKernelGGL(sf_resolve_kernel, dim3((h * w + SF_THREADS - 1) / SF_THREADS, B), dim3(SF_THREADS), 0, stream,
                     (const unsigned long long*)keys, pts, normals, pose, attr, C, N, h, w, fill, index_map, depth_map, normal_map, attr_map,
                     counts);
  return cmr_launch_status();
}

extern "C" int cmr_depth_test_f32(const float* pts, const void* mask, int mask_bytes, const float* pose, const float* K, const float* Z, int B,
                                  int N, int h, int w, int radius, float rel_tol, float abs_tol, uint8_t* visible, int32_t* counts,
                                  hipStream_t stream) {
  CMR_REQUIRE(pts && mask && pose && K && Z && visible && counts);
  CMR_REQUIRE(cmr_cloud_map_ok(B, N, h, w) && cmr_mask_bytes_ok(mask_bytes));
  CMR_REQUIRE(radius >= 0 && radius <= CMR_MAX_RADIUS);
  CMR_REQUIRE(cmr_tols_ok(rel_tol, abs_tol));
  CMR_REQUIRE(cmr_aligned4(Z));
  const float opr = cmr_one_plus(rel_tol);
  hipLaunchKernelGGL(cmr_zero_kernel<SF_THREADS>, dim3(1), dim3(SF_THREADS), 0, stream, counts, 3 * B);
  hipLaunchKernelGGL(sf_test_kernel, dim3((N + SFT_ROWS - 1) / SFT_ROWS, B), dim3(SF_THREADS), 0, stream, pts, mask, mask_bytes, pose, K, Z, N,
                     h, w, radius, opr, abs_tol, visible, counts);
  return cmr_launch_status();
}
