// Pose-guided matching (port extension): the nearest pixel feature of every selected point INSIDE a window round the
// point's projection under a given pose, instead of cmr_feat_match_f32's sweep over all h*w pixels.
//
// Two launches on the caller's stream (plus one memset of the counts):
//   gm_project_kernel  one thread per row: X_c = R x + t, p = K X_c, (u, v) = (p0 / p2, p1 / p2) in fp32, centre = rint; decides "in
//                      view" on the floats, writes proj, the fill values of the rows that are not in view (idx -1, dist NaN, keep 0),
//                      counts the selected rows and appends the in-view rows (row number + integer centre) to the sample's list.  The
//                      list position comes from one integer atomic per wave on counts[b][1], so the ORDER of the list is free -- no
//                      output depends on it: every row's results are written by the one 16-lane group that owns the row.
//   gm_match_kernel    a 16-lane group per listed row, four groups per wave, 16 per workgroup: lane j keeps channels 4j .. 4j+3 of the
//                      point feature in registers; for every window pixel in increasing p (dy outer, dx inner) the group reads the
//                      pixel's 256-byte row as ONE coalesced float4-per-lane load, takes the direct sum of squared differences and
//                      keeps the minimum with a strict <, so the lowest p of a tie stays.  Workgroups past the sample's in-view count
//                      (read on the device) return at once: the time follows the in-view rows and (2r + 1)^2, not h*w.
// Summation order of one distance: lane j: s = d0*d0, then fma(d1, d1, s), fma(d2, d2, s), fma(d3, d3, s) over its channels 4j .. 4j+3;
// then a butterfly over the 16 lanes on the DPP data path (lane ^ 1, lane ^ 2, row_half_mirror, row_mirror), i.e. the balanced tree
// ((s0 + s1) + (s2 + s3)) + ... ; IEEE addition commutes, so all 16 lanes hold the same bits.  dist = sqrtf of that minimum.
// The loop bounds are wave-uniform (every group walks the whole (2r + 1)^2 square); a pixel outside the map is read from the clamped
// address and its score discarded, so there is no divergent branch and no partial EXEC under the DPP moves.
#include "cmr_project.h"

namespace {

constexpr int GM_C = 64;            // feature width (the model's only one)
constexpr int GM_THREADS = 256;     // 4 waves
constexpr int GM_LANES = 16;        // lanes per row: 16 x float4 = one 256-byte feature row
constexpr int GM_ROWS = GM_THREADS / GM_LANES;   // rows per workgroup
constexpr int GM_AHEAD = 4;         // window pixels whose loads are in flight together per group

__global__ __launch_bounds__(256) void gm_project_kernel(const float* __restrict__ pts, const void* __restrict__ mask, int mask_bytes,
                                                         const float* __restrict__ pose, const float* __restrict__ Kin, int N, int h,
                                                         int w, int radius, int32_t* __restrict__ idx, float* __restrict__ dist,
                                                         uint8_t* __restrict__ keep, float* __restrict__ proj,
                                                         int32_t* __restrict__ counts, int32_t* __restrict__ list,
                                                         int2* __restrict__ centre) {
  const int b = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  const int64_t g = (int64_t)b * N + n;
  const bool sel = n < N && cmr_sel(mask, mask_bytes, g);
  bool view = false;
  int cxi = 0, cyi = 0;
  if (sel) {
    const CmrProj p = cmr_project(pose + 16 * b, Kin + 9 * b, pts + (int64_t)b * 3 * N, N, n, h, w, radius);
    view = p.view;
    cxi = p.cx;
    cyi = p.cy;
    if (proj) { proj[(int64_t)b * 2 * N + n] = p.u; proj[(int64_t)b * 2 * N + N + n] = p.v; }
  } else if (n < N && proj) {
    proj[(int64_t)b * 2 * N + n] = __builtin_nanf("");
    proj[(int64_t)b * 2 * N + N + n] = __builtin_nanf("");
  }
  if (n < N && !view) {
    idx[g] = -1;
    keep[g] = 0;
    if (dist) dist[g] = __builtin_nanf("");
  }
  const unsigned long long bs = __ballot(sel), bv = __ballot(view);
  int base = 0;
  if (lane == 0) {
    if (bs) atomicAdd(&counts[4 * b], __popcll(bs));
    if (bv) base = atomicAdd(&counts[4 * b + 1], __popcll(bv));
  }
  base = __shfl(base, 0);
  if (view) {
    const int pos = base + __popcll(bv & ((1ull << lane) - 1ull));
    list[(int64_t)b * N + pos] = n;
    centre[(int64_t)b * N + pos] = make_int2(cxi, cyi);
  }
}

__global__ __launch_bounds__(GM_THREADS) void gm_match_kernel(const float* __restrict__ pc, const float* __restrict__ img, int B, int N, int h,
                                                              int w, int radius, float max_dist, const float* __restrict__ gt_xy,
                                                              float thr, const int32_t* __restrict__ list,
                                                              const int2* __restrict__ centre, int32_t* __restrict__ idx,
                                                              float* __restrict__ dist, uint8_t* __restrict__ keep,
                                                              int32_t* __restrict__ counts) {
  // sample fastest: with B a multiple of 8 the workgroups of one sample land on one XCD and share its L2 copy of the sample's map
  const int b = blockIdx.x % B, grp = blockIdx.x / B;
  const int nview = counts[4 * b + 1];                 // written by gm_project_kernel (the previous launch on the stream)
  if (grp * GM_ROWS >= nview) return;
  const int q = grp * GM_ROWS + (threadIdx.x >> 4), j = threadIdx.x & 15;
  const bool active = q < nview;
  const int n = active ? list[(int64_t)b * N + q] : 0;
  const int2 c = active ? centre[(int64_t)b * N + q] : make_int2(0, 0);
  const float4 a = active ? reinterpret_cast<const float4*>(pc + ((int64_t)b * N + n) * GM_C)[j] : make_float4(0.f, 0.f, 0.f, 0.f);
  const float4* img_b = reinterpret_cast<const float4*>(img + (int64_t)b * h * w * GM_C) + j;
  float best = __builtin_huge_valf();
  int bidx = -1;
  // the window as one run of (2r + 1)^2 offsets in increasing p, GM_AHEAD pixels per step: their loads are issued together, then scored
  const int total = (2 * radius + 1) * (2 * radius + 1);
  int dx = -radius, dy = -radius;                      // wave-uniform
  for (int k = 0; k < total; k += GM_AHEAD) {
    float4 f[GM_AHEAD];
    int p[GM_AHEAD];
    bool in[GM_AHEAD];
#pragma unroll
    for (int u = 0; u < GM_AHEAD; ++u) {
      const int x = c.x + dx, y = c.y + dy;            // past the end of the run dy = r + 1: clamped like any pixel outside the map
      in[u] = k + u < total && x >= 0 && x < w && y >= 0 && y < h;
      p[u] = (y < 0 ? 0 : (y >= h ? h - 1 : y)) * w + (x < 0 ? 0 : (x >= w ? w - 1 : x));
      f[u] = img_b[(int64_t)p[u] * (GM_C / 4)];
      if (++dx > radius) { dx = -radius; ++dy; }
    }
#pragma unroll
    for (int u = 0; u < GM_AHEAD; ++u) {
      const float d0 = a.x - f[u].x, d1 = a.y - f[u].y, d2 = a.z - f[u].z, d3 = a.w - f[u].w;
      float s = d0 * d0;
      s = fmaf(d1, d1, s);
      s = fmaf(d2, d2, s);
      s = fmaf(d3, d3, s);
      s = cmr_sum16(s);
      if (bidx < 0 && in[u]) bidx = p[u];              // all-NaN scores keep the window's first pixel, as torch.argmin
      if (in[u] && s < best) { best = s; bidx = p[u]; }   // strict, p increasing: the lowest p of a tie stays
    }
  }
  bool kept = false, inl = false;
  if (active && j == 0) {
    const int64_t g = (int64_t)b * N + n;
    const float d = sqrtf(best);
    kept = !(max_dist > 0.f) || d <= max_dist;
    idx[g] = bidx;
    keep[g] = kept ? 1 : 0;
    if (dist) dist[g] = d;
    if (gt_xy) {
      const float x = gt_xy[(int64_t)b * 2 * N + n], y = gt_xy[(int64_t)b * 2 * N + N + n];
      const float ex = (float)(bidx % w) - x, ey = (float)(bidx / w) - y;
      inl = isfinite(x) && isfinite(y) && sqrtf(ex * ex + ey * ey) <= thr;
    }
  }
  const int c2 = __popcll(__ballot(kept)), c3 = __popcll(__ballot(kept && inl));
  if ((threadIdx.x & 63) == 0) {
    if (c2) atomicAdd(&counts[4 * b + 2], c2);
    if (c3) atomicAdd(&counts[4 * b + 3], c3);
  }
}

}  // namespace

extern "C" int64_t cmr_guided_match_workspace_bytes(int B, int N) {
  return B <= 0 || N <= 0 ? 0 : cmr_up16((int64_t)B * N * 4) + cmr_up16((int64_t)B * N * 8);
}

extern "C" int cmr_guided_match_f32(const float* pts, const float* pc_feat, const float* img_feat, int C, int B, int N, int h, int w,
                                    const void* mask, int mask_bytes, const float* pose, const float* K, int radius, float max_dist,
                                    const float* gt_xy, float thr, int32_t* idx, uint8_t* keep, int32_t* counts, float* dist, float* proj,
                                    void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  CMR_REQUIRE(pts && pc_feat && img_feat && mask && pose && K && idx && keep && counts && workspace);
  CMR_REQUIRE(C == GM_C && cmr_cloud_map_ok(B, N, h, w));
  CMR_REQUIRE(mask_bytes == 1 || mask_bytes == 8);
  CMR_REQUIRE(radius >= 0 && radius <= CMR_MAX_RADIUS && max_dist >= 0.f && __builtin_isfinite(max_dist));
  CMR_REQUIRE(cmr_aligned16(pc_feat) && cmr_aligned16(img_feat) && cmr_aligned16(workspace));
  CMR_REQUIRE(workspace_bytes >= cmr_guided_match_workspace_bytes(B, N));
  const int64_t groups = ((int64_t)N + GM_ROWS - 1) / GM_ROWS * B;
  CMR_REQUIRE(groups <= 0x7fffffff);
  int32_t* list = (int32_t*)workspace;
  int2* centre = (int2*)((char*)workspace + cmr_up16((int64_t)B * N * 4));
  if (hipMemsetAsync(counts, 0, (size_t)B * 4 * sizeof(int32_t), stream) != hipSuccess) return CMR_ELAUNCH;
  hipLaunchKernelGGL(gm_project_kernel, dim3((N + 255) / 256, B), dim3(256), 0, stream, pts, mask, mask_bytes, pose, K, N, h, w, radius, idx,
                     dist, keep, proj, counts, list, centre);
  hipLaunchKernelGGL(gm_match_kernel, dim3((unsigned)groups), dim3(GM_THREADS), 0, stream, pc_feat, img_feat, B, N, h, w, radius, max_dist,
                     gt_xy, thr, (const int32_t*)list, (const int2*)centre, idx, dist, keep, counts);
  return cmr_launch_status();
}
