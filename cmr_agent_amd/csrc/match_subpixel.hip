// Sub-pixel match positions (port extension): turns the pixel index any of the matchers returns (cmr_feat_match_f32,
// cmr_feat_match_filter_f32, cmr_guided_match_f32) into a float position by fitting a parabola through the squared feature distances of
// the matched pixel and its two neighbours, separately along x and along y.
//
// One launch on the caller's stream (plus one memset of the counts):
//   ms_subpixel_kernel  a 16-lane group per row, four groups per wave as gm_match_kernel, 64 per 1024-thread workgroup: lane j keeps
//                       channels 4j .. 4j+3 of the point feature in registers and reads the matched pixel p and p - 1, p + 1, p - w,
//                       p + w as one coalesced float4-per-lane load each (a 256-byte row per group), all issued before the first is
//                       scored.  A neighbour outside the map reads the clamped address (p itself) and an unmatched row reads nothing;
//                       both predicates are uniform over the 16 lanes of a group, so every DPP move has all its source lanes.
// Summation order of one squared distance (guided_match.hip's): lane j: s = d0*d0, then fma(d1, d1, s), fma(d2, d2, s), fma(d3, d3, s)
// over its channels 4j .. 4j+3; then the butterfly over the 16 lanes on the DPP data path (lane ^ 1, lane ^ 2, row_half_mirror,
// row_mirror), the balanced tree ((s0 + s1) + (s2 + s3)) + ...; all 16 lanes hold the same bits.  Per axis num = sm - sp, den =
// (sm - s0) + (sp - s0), delta = 0.5f * num / den (IEEE division), clamped to [-0.5, 0.5]; uv = (float)x + delta.
// counts: the four flags of a row are reduced inside the workgroup (one ballot per wave and word, 64 words of LDS) and the workgroup
// issues at most one integer atomic per word; every uv element is a plain store by the group that owns the row.  The atomics on a
// sample's count words serialise at ~48 ns each on the MI355X and bound the kernel: hence 64 rows per workgroup, not 16.
#include "cmr_common.h"

namespace {

constexpr int MS_C = 64;            // feature width (the model's only one)
constexpr int MS_THREADS = 1024;    // 16 waves
constexpr int MS_LANES = 16;        // lanes per row: 16 x float4 = one 256-byte feature row
constexpr int MS_ROWS = MS_THREADS / MS_LANES;   // rows per workgroup

template <int CTRL>
__device__ __forceinline__ float ms_dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}

// squared distance of the group's point feature and one pixel row: the lane's four channels, then the sum over the 16 lanes of a DPP row
__device__ __forceinline__ float ms_sqdist(const float4& a, const float4& f) {
  const float d0 = a.x - f.x, d1 = a.y - f.y, d2 = a.z - f.z, d3 = a.w - f.w;
  float s = d0 * d0;
  s = fmaf(d1, d1, s);
  s = fmaf(d2, d2, s);
  s = fmaf(d3, d3, s);
  s += ms_dpp<0xB1>(s);             // quad_perm:[1,0,3,2]
  s += ms_dpp<0x4E>(s);             // quad_perm:[2,3,0,1]
  s += ms_dpp<0x141>(s);            // row_half_mirror
  s += ms_dpp<0x140>(s);            // row_mirror
  return s;
}

// the vertex of the parabola through (-1, sm), (0, s0), (+1, sp); fitted only for a strict finite minimum
__device__ __forceinline__ float ms_vertex(bool in_map, float s0, float sm, float sp, bool& fitted) {
  const float num = sm - sp, den = (sm - s0) + (sp - s0);
  fitted = in_map && isfinite(num) && isfinite(den) && den > 0.f;
  const float d = 0.5f * num / den;
  return fitted ? fminf(fmaxf(d, -0.5f), 0.5f) : 0.f;
}

__global__ __launch_bounds__(MS_THREADS) void ms_subpixel_kernel(const float* __restrict__ pc, const float* __restrict__ img, int B, int N,
                                                                 int h, int w, const int32_t* __restrict__ idx,
                                                                 const void* __restrict__ mask, int mask_bytes,
                                                                 const float* __restrict__ gt_xy, float thr, float* __restrict__ uv,
                                                                 int32_t* __restrict__ counts) {
  __shared__ int32_t part[MS_THREADS / 64][4];
  // sample fastest, as gm_match_kernel: with B a multiple of 8 the workgroups of one sample land on one XCD and share its L2 copy of the map
  const int b = blockIdx.x % B, grp = blockIdx.x / B;
  const int n = grp * MS_ROWS + (threadIdx.x >> 4), j = threadIdx.x & 15;
  const bool valid = n < N;
  const int64_t g = (int64_t)b * N + (valid ? n : N - 1);
  const int32_t pi = idx[g];                                       // issued beside the mask read, not behind it
  const bool sel = cmr_sel_or_all(mask, mask_bytes, g);
  const bool matched = valid && sel && pi >= 0 && pi < h * w;      // an index outside the map is never dereferenced
  const int p = matched ? pi : 0;
  const int x = p % w, y = p / w;
  const bool in_x = x >= 1 && x <= w - 2, in_y = y >= 1 && y <= h - 2;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  const float4* img_b = reinterpret_cast<const float4*>(img + (int64_t)b * h * w * MS_C) + j;
  const int dxo = in_x ? 1 : 0, dyo = in_y ? w : 0;                // out-of-map neighbours: the clamped address, the score is discarded
  float4 a = zero, f0 = zero, fl = zero, fr = zero, fu = zero, fd = zero;
  if (matched) {                                                   // uniform over the group's 16 lanes
    a = reinterpret_cast<const float4*>(pc + g * MS_C)[j];
    f0 = img_b[(int64_t)p * (MS_C / 4)];
    fl = img_b[(int64_t)(p - dxo) * (MS_C / 4)];
    fr = img_b[(int64_t)(p + dxo) * (MS_C / 4)];
    fu = img_b[(int64_t)(p - dyo) * (MS_C / 4)];
    fd = img_b[(int64_t)(p + dyo) * (MS_C / 4)];
  }
  const float s0 = ms_sqdist(a, f0);
  const float sl = ms_sqdist(a, fl), sr = ms_sqdist(a, fr), su = ms_sqdist(a, fu), sd = ms_sqdist(a, fd);
  bool fit_x, fit_y;
  const float ddx = ms_vertex(in_x, s0, sl, sr, fit_x), ddy = ms_vertex(in_y, s0, su, sd, fit_y);
  const bool lead = valid && j == 0;
  bool both = false, inl_int = false, inl_sub = false;
  if (lead) {
    const float nanv = __builtin_nanf("");
    const float xi = (float)x, yi = (float)y, xs = xi + ddx, ys = yi + ddy;
    float* o = uv + (int64_t)b * 2 * N;
    o[n] = matched ? xs : nanv;
    o[N + n] = matched ? ys : nanv;
    both = matched && fit_x && fit_y;
    if (gt_xy && matched) {
      const float gx = gt_xy[(int64_t)b * 2 * N + n], gy = gt_xy[(int64_t)b * 2 * N + N + n];
      const bool fin = isfinite(gx) && isfinite(gy);
      const float ex = xi - gx, ey = yi - gy, fx = xs - gx, fy = ys - gy;
      inl_int = fin && sqrtf(ex * ex + ey * ey) <= thr;
      inl_sub = fin && sqrtf(fx * fx + fy * fy) <= thr;
    }
  }
  const int c0 = __popcll(__ballot(lead && matched)), c1 = __popcll(__ballot(both));
  const int c2 = __popcll(__ballot(inl_int)), c3 = __popcll(__ballot(inl_sub));
  if ((threadIdx.x & 63) == 0) {
    int32_t* q = part[threadIdx.x >> 6];
    q[0] = c0; q[1] = c1; q[2] = c2; q[3] = c3;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    int t = 0;
#pragma unroll
    for (int v = 0; v < MS_THREADS / 64; ++v) t += part[v][threadIdx.x];
    if (t) atomicAdd(&counts[4 * b + threadIdx.x], t);
  }
}

}  // namespace

extern "C" int cmr_match_subpixel_f32(const float* pc_feat, const float* img_feat, int C, int B, int N, int h, int w, const int32_t* idx,
                                      const void* mask, int mask_bytes, const float* gt_xy, float thr, float* uv, int32_t* counts,
                                      hipStream_t stream) {
  CMR_REQUIRE(pc_feat && img_feat && idx && uv && counts);
  CMR_REQUIRE(B > 0 && B <= 65535 && N > 0 && h > 0 && w > 0 && (int64_t)h * w <= (int64_t)1 << 24);
  if (C != MS_C) return CMR_EUNSUPPORTED;
  CMR_REQUIRE((int64_t)N <= (int64_t)65535 * 256);
  CMR_REQUIRE(!mask || mask_bytes == 1 || mask_bytes == 8);
  CMR_REQUIRE(cmr_aligned16(pc_feat) && cmr_aligned16(img_feat));
  const int64_t groups = ((int64_t)N + MS_ROWS - 1) / MS_ROWS * B;
  CMR_REQUIRE(groups <= 0x7fffffff);
  if (hipMemsetAsync(counts, 0, (size_t)B * 4 * sizeof(int32_t), stream) != hipSuccess) return CMR_ELAUNCH;
  hipLaunchKernelGGL(ms_subpixel_kernel, dim3((unsigned)groups), dim3(MS_THREADS), 0, stream, pc_feat, img_feat, B, N, h, w, idx, mask,
                     mask_bytes, gt_xy, thr, uv, counts);
  return cmr_launch_status();
}
