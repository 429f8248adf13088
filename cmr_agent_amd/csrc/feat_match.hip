// Nearest pixel feature of every selected point feature, with the inlier counts of the geometric model's match evaluation
// (reference MultiHeadModel.py:180-216, 285-315 and Test_Geo.py:91-122: argmin over the h*w pixels of the L2 distance, 64 channels).
//
// Two launches, both enqueued on the caller's stream:
//   fm_compact_kernel  selected rows of every sample -> a row list in the workspace (order free: every result is written per row),
//                      its length into counts[b][0] (= the number of selected points), idx = -1 / dist = NaN on unselected rows;
//   fm_match_kernel    a workgroup takes 256 listed rows (4 waves x 2 column tiles of 32) and streams the sample's pixel features
//                      through LDS in tiles of 64; the score |q|^2 - 2 p.q is a 32x32x2 fp32 MFMA product (pixels = A rows, points =
//                      B columns, so a point's 32 candidates of a tile sit in one lane's 16 accumulators x 2 lane halves) and the
//                      running (min, index) stays in registers; workgroups past the list's length return at once.
// Compacting first makes an unselected row cost one mask read: with ~30-60 % of the rows selected, a 256-row tile is almost never
// empty, so skipping empty tiles would save nothing ("Match evaluation").
#include "cmr_common.h"

namespace {

constexpr int FM_C = 64;         // feature width (the model's only one)
constexpr int FM_THREADS = 256;  // 4 waves
constexpr int FM_ROWS = 256;     // listed rows per workgroup: wave w holds rows 64w .. 64w+63 as two 32-column B tiles
constexpr int FM_PX = 64;        // pixels per LDS tile: 64 rows of 16 float4 chunks, chunk c of row r stored at c ^ (r & 15)

__device__ __forceinline__ unsigned fm_xhalf_u(unsigned u) {
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return (threadIdx.x & 32) ? r[0] : r[1];
}

__global__ __launch_bounds__(256) void fm_compact_kernel(const void* __restrict__ mask, int mask_bytes, int N, int32_t* __restrict__ list,
                                                         int32_t* __restrict__ idx, float* __restrict__ dist, int32_t* __restrict__ counts) {
  const int b = blockIdx.y;
  const int n = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int64_t g = (int64_t)b * N + n;
  bool sel = false;
  if (n < N) {
    sel = cmr_sel(mask, mask_bytes, g);
    if (!sel) {
      idx[g] = -1;
      if (dist) dist[g] = __builtin_nanf("");
    }
  }
  const unsigned long long bal = __ballot(sel);
  const int cnt = __popcll(bal);
  int base = 0;
  if (lane == 0 && cnt) base = atomicAdd(&counts[4 * b], cnt);
  base = __shfl(base, 0);
  if (sel) list[(int64_t)b * N + base + __popcll(bal & ((1ull << lane) - 1ull))] = n;
}

// Stages pixels [p0, p0 + 64) of one sample: thread t loads a quarter row (4 float4) of pixel t >> 2 into registers.
__device__ __forceinline__ void fm_load(const float* __restrict__ img, int hw, int p0, float4 (&v)[4]) {
  const int p = p0 + (threadIdx.x >> 2);
  if (p < hw) {
    const float4* src = reinterpret_cast<const float4*>(img + (int64_t)p * FM_C) + 4 * (threadIdx.x & 3);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = src[i];
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// ... and writes them (swizzled) plus the pixel's squared norm; pixels past the map get +inf and are never chosen.
__device__ __forceinline__ void fm_store(float4* tile, float* qn, int hw, int p0, const float4 (&v)[4]) {
  const int r = threadIdx.x >> 2, q = threadIdx.x & 3;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    tile[r * 16 + ((4 * q + i) ^ (r & 15))] = v[i];
    s = fmaf(v[i].x, v[i].x, s);
    s = fmaf(v[i].y, v[i].y, s);
    s = fmaf(v[i].z, v[i].z, s);
    s = fmaf(v[i].w, v[i].w, s);
  }
  s += __shfl_xor(s, 1);
  s += __shfl_xor(s, 2);
  if (q == 0) qn[r] = p0 + r < hw ? s : __builtin_huge_valf();
}

__global__ __launch_bounds__(256) void fm_match_kernel(const float* __restrict__ pc, const float* __restrict__ img, const int32_t* __restrict__ list,
                                                       int N, int hw, int w, const float* __restrict__ gt_xy, float thr,
                                                       const uint8_t* __restrict__ img_ov, int32_t* __restrict__ idx, float* __restrict__ dist,
                                                       int32_t* __restrict__ counts) {
  __shared__ float4 tile[2][FM_PX * 16];
  __shared__ __attribute__((aligned(16))) float qn[2][FM_PX];
  const int b = blockIdx.y;
  const int nsel = counts[4 * b];                                   // written by fm_compact_kernel (previous launch on the stream)
  const int row0 = blockIdx.x * FM_ROWS;
  if (row0 >= nsel) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int half = lane >> 5, col = lane & 31;
  const float* img_b = img + (int64_t)b * hw * FM_C;

  // B operand: lane holds features 32*half .. 32*half+31 of its column's point (k of MFMA step s is 32*half + s, on both operands)
  float bq[2][32];
  int n_of[2];
  bool valid[2];
  float pn[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int r = row0 + 64 * wave + 32 * t + col;
    valid[t] = r < nsel;
    n_of[t] = valid[t] ? list[(int64_t)b * N + r] : 0;
    const float4* src = reinterpret_cast<const float4*>(pc + ((int64_t)b * N + n_of[t]) * FM_C + 32 * half);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float4 v = valid[t] ? src[j] : make_float4(0.f, 0.f, 0.f, 0.f);
      bq[t][4 * j] = v.x; bq[t][4 * j + 1] = v.y; bq[t][4 * j + 2] = v.z; bq[t][4 * j + 3] = v.w;
      s = fmaf(v.x, v.x, s); s = fmaf(v.y, v.y, s); s = fmaf(v.z, v.z, s); s = fmaf(v.w, v.w, s);
    }
    pn[t] = s + cmr_xhalf(s);
  }

  float best[2] = {__builtin_huge_valf(), __builtin_huge_valf()};
  int bidx[2] = {0, 0};                                           // all-NaN scores keep pixel 0, as torch.argmin
  const int ntile = (hw + FM_PX - 1) / FM_PX;
  float4 pre[4];
  fm_load(img_b, hw, 0, pre);
  fm_store(tile[0], qn[0], hw, 0, pre);
  __syncthreads();
  for (int it = 0; it < ntile; ++it) {
    const int buf = it & 1, p0 = it * FM_PX;
    const bool more = it + 1 < ntile;
    if (more) fm_load(img_b, hw, p0 + FM_PX, pre);
#pragma unroll 1
    for (int u = 0; u < 2; ++u) {                                  // two 32-pixel sub-tiles
      const int pr = 32 * u + col;
      float a[32];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float4 v = tile[buf][pr * 16 + ((8 * half + j) ^ (pr & 15))];
        a[4 * j] = v.x; a[4 * j + 1] = v.y; a[4 * j + 2] = v.z; a[4 * j + 3] = v.w;
      }
      f32x16 acc0 = {}, acc1 = {};
#pragma unroll
      for (int s = 0; s < 32; ++s) {
        acc0 = cmr_mfma32(a[s], bq[0][s], acc0);
        acc1 = cmr_mfma32(a[s], bq[1][s], acc1);
      }
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const float4 q4 = *reinterpret_cast<const float4*>(&qn[buf][32 * u + 8 * g4 + 4 * half]);
        const float qv[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int g = 4 * g4 + e;
          const int pix = p0 + 32 * u + 8 * g4 + 4 * half + e;       // = cmr_mfma_row(g, lane): increasing with g in a lane
          const float v0 = fmaf(-2.f, acc0[g], qv[e]);
          const float v1 = fmaf(-2.f, acc1[g], qv[e]);
          if (v0 < best[0]) { best[0] = v0; bidx[0] = pix; }        // strict: the first (lowest) pixel of a tie stays
          if (v1 < best[1]) { best[1] = v1; bidx[1] = pix; }
        }
      }
    }
    if (more) fm_store(tile[buf ^ 1], qn[buf ^ 1], hw, p0 + FM_PX, pre);
    __syncthreads();
  }

  // the two lane halves saw interleaved pixel rows: lower score wins, a tie goes to the lower pixel index
  bool inl[2], ov[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const float ob = __builtin_bit_cast(float, fm_xhalf_u(__builtin_bit_cast(unsigned, best[t])));
    const int oi = (int)fm_xhalf_u((unsigned)bidx[t]);
    if (ob < best[t] || (ob == best[t] && oi < bidx[t])) { best[t] = ob; bidx[t] = oi; }
    const bool mine = valid[t] && half == 0;
    const int64_t g = (int64_t)b * N + n_of[t];
    inl[t] = false;
    ov[t] = false;
    if (mine) {
      const int p = bidx[t];
      idx[g] = p;
      if (dist) dist[g] = sqrtf(fmaxf(pn[t] + best[t], 0.f));
      if (gt_xy) {
        const float x = gt_xy[(int64_t)b * 2 * N + n_of[t]], y = gt_xy[(int64_t)b * 2 * N + N + n_of[t]];
        const float dx = (float)(p % w) - x, dy = (float)(p / w) - y;
        inl[t] = isfinite(x) && isfinite(y) && sqrtf(dx * dx + dy * dy) <= thr;
      }
      if (img_ov) ov[t] = img_ov[(int64_t)b * hw + p] != 0;
    }
  }
  const int c1 = __popcll(__ballot(inl[0])) + __popcll(__ballot(inl[1]));
  const int c2 = __popcll(__ballot(ov[0])) + __popcll(__ballot(ov[1]));
  const int c3 = __popcll(__ballot(inl[0] && ov[0])) + __popcll(__ballot(inl[1] && ov[1]));
  if (lane == 0) {
    if (c1) atomicAdd(&counts[4 * b + 1], c1);
    if (c2) atomicAdd(&counts[4 * b + 2], c2);
    if (c3) atomicAdd(&counts[4 * b + 3], c3);
  }
}

}  // namespace

extern "C" int64_t cmr_feat_match_workspace_bytes(int B, int N) {
  return B <= 0 || N <= 0 ? 0 : (int64_t)B * N * (int64_t)sizeof(int32_t);
}

extern "C" int cmr_feat_match_f32(const float* pc_feat, const float* img_feat, int C, int B, int N, int h, int w, const void* mask,
                                  int mask_bytes, const float* gt_xy, float thr, const uint8_t* img_overlap, int32_t* idx, float* dist,
                                  int32_t* counts, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  CMR_REQUIRE(pc_feat && img_feat && mask && idx && counts && workspace);
  CMR_REQUIRE(C == FM_C && B > 0 && B <= 65535 && N > 0 && h > 0 && w > 0 && (int64_t)h * w <= (int64_t)1 << 30);
  CMR_REQUIRE(mask_bytes == 1 || mask_bytes == 8);
  CMR_REQUIRE(cmr_aligned16(pc_feat) && cmr_aligned16(img_feat));
  CMR_REQUIRE(workspace_bytes >= cmr_feat_match_workspace_bytes(B, N));
  int32_t* list = (int32_t*)workspace;
  if (hipMemsetAsync(counts, 0, (size_t)B * 4 * sizeof(int32_t), stream) != hipSuccess) return CMR_ELAUNCH;
  hipLaunchKernelGGL(fm_compact_kernel, dim3((N + 255) / 256, B), dim3(256), 0, stream, mask, mask_bytes, N, list, idx, dist, counts);
  hipLaunchKernelGGL(fm_match_kernel, dim3((N + FM_ROWS - 1) / FM_ROWS, B), dim3(FM_THREADS), 0, stream, pc_feat, img_feat,
                     (const int32_t*)list, N, h * w, w, gt_xy, thr, img_overlap, idx, dist, counts);
  return cmr_launch_status();
}
