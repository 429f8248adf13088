// Pre-LN transformer block (reference models/ImageViT.py:61-158, PointViT.py:96-183, IMGPCEncoder.py:14-102) in three
// launches instead of seven to nine:
//
//   cmr_ln64_linear_f32      LayerNorm(64) + projection for up to two row sets in ONE launch
//                            (self block: x -> [q|k|v];  cross block: x -> q and y -> [k|v], same norm)
//   cmr_mha_f32              (attention.hip, unchanged)
//   cmr_vit_out_ffn_f32      x1 = ctx Wo + bo + x ;  out = x1 + W2 gelu(W1 LN(x1) + b1) + b2
//
// The token counts of this path are small (B*T = 3 344 image proxies, B*Q = 2 048 point proxies): the unfused block
// is a chain of launch-latency-bound kernels, each filling a fraction of the chip.  Weights are passed as MFMA A
// fragments ([n_out/32][k/8][64 lanes][4], cmr_agent_amd/models/_pack.py:frag_pack) and read straight from L2 with
// 1 KB coalesced wave loads; everything is computed transposed (D'[channel][row]: a lane owns one row, accumulator
// register 4q+e of tile t is channel 32t + 8q + 4h + e = B fragment k-group 4t+q of the next GEMM).
// The MLP kernel gives one 32-row tile to a workgroup of 8 waves: every wave redoes the small out-projection and
// LayerNorm, takes 128 of the 1024 hidden units through fc1 / GELU / its K-slice of fc2, and the 8 partial outputs
// are summed through LDS in a fixed order.
#include "cmr_mfma16.h"

namespace {

// acc[t] = sum_kg sum_j Wf[tile0 + t][kg0 + kg][lane][j] * bfrag(kg, j).  The fragments come straight from L2
// (~1-2 us under load) and a k-group is only T*4 MFMAs (0.25-0.5 us), so they are requested D k-groups ahead
// through a register ring; with one k-group of lookahead every step of the chain was an exposed L2 round trip.
template <int T, int KG, int D, typename BF>
__device__ __forceinline__ void vf_gemm(const float* __restrict__ wf, int kg_total, int tile0, int kg0, int lane,
                                        f32x16 (&acc)[T], BF bfrag) {
  static_assert(D >= 1 && D <= KG, "prefetch depth");
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  const float* wp = wf + ((int64_t)tile0 * kg_total + kg0) * 256 + lane * 4;
  const int64_t tstride = (int64_t)kg_total * 256;
  f32x4 ring[D][T];
#pragma unroll
  for (int d = 0; d < D; ++d)
#pragma unroll
    for (int t = 0; t < T; ++t) ring[d][t] = *reinterpret_cast<const f32x4*>(wp + t * tstride + d * 256);
#pragma unroll
  for (int kg = 0; kg < KG; ++kg) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float b = bfrag(kg, j);
#pragma unroll
      for (int t = 0; t < T; ++t) acc[t] = cmr_mfma32(ring[kg % D][t][j], b, acc[t]);
    }
    if (kg + D < KG) {
#pragma unroll
      for (int t = 0; t < T; ++t) ring[kg % D][t] = *reinterpret_cast<const f32x4*>(wp + t * tstride + (kg + D) * 256);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

struct LnLinProblem {
  const float* x; int64_t ldx; uint32_t rows;
  const float* wf; const float* bias; int npair;       // n_out = 64 * npair
  float* y; int64_t ldy;
};
struct LnLinArgs {
  LnLinProblem p[2];
  uint32_t tiles0, tiles;                              // tiles of problem 0, total tiles
  const float* g; const float* b; float eps;
};

__global__ __launch_bounds__(256) void ln64_linear_kernel(const LnLinArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int h = lane >> 5, l31 = lane & 31;
  const uint32_t gt = blockIdx.x * (blockDim.x >> 6) + wave;       // one tile per wave; 1 or 4 waves per workgroup
  if (gt >= a.tiles) return;
  const LnLinProblem& P = gt < a.tiles0 ? a.p[0] : a.p[1];
  const uint32_t tile = gt < a.tiles0 ? gt : gt - a.tiles0;
  const uint32_t row = tile * 32 + l31;
  const bool valid = row < P.rows;
  const float* xp = P.x + (int64_t)(valid ? row : 0) * P.ldx + 4 * h;
  f32x4 xf[8];
#pragma unroll
  for (int kg = 0; kg < 8; ++kg) xf[kg] = *reinterpret_cast<const f32x4*>(xp + kg * 8);
  cmr_layernorm64(xf, a.g, a.b, a.eps, [&](int kg) { return 8 * kg + 4 * h; });
  for (int pr = 0; pr < P.npair; ++pr) {               // 64 output channels per pass
    f32x16 acc[2];
    vf_gemm<2, 8, 8>(P.wf, 8, 2 * pr, 0, lane, acc, [&](int kg, int j) { return xf[kg][j]; });
    f32x4 ov[8];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        const f32x4 bv = *reinterpret_cast<const f32x4*>(P.bias + 64 * pr + 32 * t + 8 * qd + 4 * h);
#pragma unroll
        for (int e = 0; e < 4; ++e) ov[4 * t + qd][e] = acc[t][4 * qd + e] + bv[e];
      }
#pragma unroll
    for (int i = 0; i < 8; ++i) cmr_pin(ov[i]);
    if (valid) {
      float* yp = P.y + (int64_t)row * P.ldy + 64 * pr + 4 * h;
#pragma unroll
      for (int i = 0; i < 8; ++i) *reinterpret_cast<f32x4*>(yp + 8 * i) = ov[i];
    }
  }
}

struct OutFfnArgs {
  const float* ctx; int64_t ldc;
  const float* x; int64_t ldx;                         // residual stream
  const float* wo_f; const float* bo;                  // [2][8][64][4], [64]
  const float* g2; const float* b2n; float eps;        // ffn_norm
  const float* w1_f; const float* b1;                  // [32][8][64][4], [1024]
  const float* w2_f; const float* b2;                  // [2][128][64][4], [64]
  float* out; int64_t ldo; uint32_t rows;
};

__global__ __launch_bounds__(512) void vit_out_ffn_kernel(const OutFfnArgs a) {
  __shared__ __attribute__((aligned(16))) float red[7 * 8 * 64 * 4];     // partial outputs of waves 1..7: [w][frag][lane][4]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int h = lane >> 5, l31 = lane & 31;
  const uint32_t row = blockIdx.x * 32 + l31;
  const bool valid = row < a.rows;
  const uint32_t rowc = valid ? row : 0;
  const float* cp = a.ctx + (int64_t)rowc * a.ldc + 4 * h;
  const float* xp = a.x + (int64_t)rowc * a.ldx + 4 * h;
  f32x4 cf[8], x1[8];
#pragma unroll
  for (int kg = 0; kg < 8; ++kg) {
    cf[kg] = *reinterpret_cast<const f32x4*>(cp + kg * 8);
    x1[kg] = *reinterpret_cast<const f32x4*>(xp + kg * 8);
  }
  // ---- x1 = ctx Wo + bo + x     (every wave: 64 MFMAs, cheaper than a broadcast through LDS)
  {
    f32x16 acc[2];
    vf_gemm<2, 8, 8>(a.wo_f, 8, 0, 0, lane, acc, [&](int kg, int j) { return cf[kg][j]; });
#pragma unroll
    for (int kg = 0; kg < 8; ++kg) {
      const f32x4 bv = *reinterpret_cast<const f32x4*>(a.bo + 8 * kg + 4 * h);
#pragma unroll
      for (int e = 0; e < 4; ++e) x1[kg][e] = (acc[kg / 4][4 * (kg % 4) + e] + bv[e]) + x1[kg][e];
    }
  }
  f32x4 xn[8];
#pragma unroll
  for (int kg = 0; kg < 8; ++kg) xn[kg] = x1[kg];
  cmr_layernorm64(xn, a.g2, a.b2n, a.eps, [&](int kg) { return 8 * kg + 4 * h; });
  // ---- this wave's 128 hidden units: fc1 + GELU, then its K-slice of fc2
  f32x16 hid[4];
  vf_gemm<4, 8, 4>(a.w1_f, 8, 4 * wave, 0, lane, hid, [&](int kg, int j) { return xn[kg][j]; });
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
      const f32x4 bv = *reinterpret_cast<const f32x4*>(a.b1 + 128 * wave + 32 * t + 8 * qd + 4 * h);
#pragma unroll
      for (int e = 0; e < 4; ++e) hid[t][4 * qd + e] = cmr_gelu(hid[t][4 * qd + e] + bv[e]);
    }
  f32x16 part[2];
  vf_gemm<2, 16, 8>(a.w2_f, 128, 0, 16 * wave, lane, part, [&](int kg, int j) { return hid[kg / 4][4 * (kg % 4) + j]; });
  if (wave > 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const f32x4 v = {part[i / 4][4 * (i % 4)], part[i / 4][4 * (i % 4) + 1], part[i / 4][4 * (i % 4) + 2], part[i / 4][4 * (i % 4) + 3]};
      *reinterpret_cast<f32x4*>(&red[(((wave - 1) * 8 + i) * 64 + lane) * 4]) = v;
    }
  }
  __syncthreads();
  if (wave != 0) return;
  f32x4 ov[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    f32x4 s = {part[i / 4][4 * (i % 4)], part[i / 4][4 * (i % 4) + 1], part[i / 4][4 * (i % 4) + 2], part[i / 4][4 * (i % 4) + 3]};
#pragma unroll
    for (int w = 0; w < 7; ++w) s += *reinterpret_cast<const f32x4*>(&red[((w * 8 + i) * 64 + lane) * 4]);
    const f32x4 bv = *reinterpret_cast<const f32x4*>(a.b2 + 8 * i + 4 * h);
#pragma unroll
    for (int e = 0; e < 4; ++e) ov[i][e] = (s[e] + bv[e]) + x1[i][e];
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) cmr_pin(ov[i]);
  if (valid) {
    float* yp = a.out + (int64_t)row * a.ldo + 4 * h;
#pragma unroll
    for (int i = 0; i < 8; ++i) *reinterpret_cast<f32x4*>(yp + 8 * i) = ov[i];
  }
}


// ---- the same out-projection + MLP on 16-ROW tiles (v_mfma_f32_16x16x4_f32) -------------------------------------------------------
// vit_out_ffn_kernel gives a 32-row tile to one workgroup: B*T = 3 344 image proxies are 105 workgroups (2 048 point proxies: 64) and
// each SIMD holds two waves of 320 MFMAs x 64 cycles = 21 us of matrix work on 40 % of the chip.  With 16x16x4 MFMAs (same FLOP
// rate, half the rows per tile) the same block is 209 / 128 workgroups of 10 us each.  Operand layout of 16x16x4 with the weights as
// A: lane = 16 g + m supplies W[m][4 ks + g]; activations as B: lane = 16 g + n supplies x[row n][4 ks + g]; D: lane holds channels
// 4 g + r (r = 0..3) of row n.  A lane therefore owns ONE row and, of every 16-channel tile T, the channels 16 T + 4 g + r -- which is
// again the B operand of k-steps (T, r) of the next GEMM when its weights are stored in that order ([n_out/16][k/16][64 lanes][4],
// lane = 16 g + m holding W[16 To + m][16 T + 4 g + r], r = 0..3: cmr_agent_amd/models/_pack.py:frag_pack16).  Rows read from memory
// are read in the same order (float4 at channel 16 T + 4 g).  The MFMA, its ring-buffered GEMM and the four-group sum: cmr_mfma16.h.
#ifdef CMR_FFN_STAMPS
#define FFN_STAMP(i) do { uint64_t t_; asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); st_[i] = t_; } while (0)
#else
#define FFN_STAMP(i) do { } while (0)
#endif
__global__ __launch_bounds__(512) void vit_out_ffn16_kernel(const OutFfnArgs a) {
  __shared__ __attribute__((aligned(16))) float red[7 * 4 * 64 * 4];     // partial outputs of waves 1..7: [w][tile][lane][4]
#ifdef CMR_FFN_STAMPS
  uint64_t st_[9];
#endif
  FFN_STAMP(0);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, n = lane & 15;
  const uint32_t row = blockIdx.x * 16 + n;
  const bool valid = row < a.rows;
  const uint32_t rowc = valid ? row : 0;
  const float* cp = a.ctx + (int64_t)rowc * a.ldc + 4 * g;
  const float* xp = a.x + (int64_t)rowc * a.ldx + 4 * g;
  f32x4 cf[4], x1[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    cf[t] = *reinterpret_cast<const f32x4*>(cp + 16 * t);
    x1[t] = *reinterpret_cast<const f32x4*>(xp + 16 * t);
  }
  FFN_STAMP(1);
  // ---- x1 = ctx Wo + bo + x     (every wave: 64 MFMAs)
  {
    f32x4 acc[4];
    m16_gemm<4, 4, 4>(a.wo_f, 4, 0, 0, lane, acc, [&](int t, int r) { return cf[t][r]; });
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const f32x4 bv = *reinterpret_cast<const f32x4*>(a.bo + 16 * t + 4 * g);
#pragma unroll
      for (int e = 0; e < 4; ++e) x1[t][e] = (acc[t][e] + bv[e]) + x1[t][e];
    }
  }
  FFN_STAMP(2);
  // ---- LayerNorm(64) of the row: 16 channels here, the others in the three partner lanes
  f32x4 xn[4];
  {
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) s += (x1[t][0] + x1[t][1]) + (x1[t][2] + x1[t][3]);
    const float mean = m16_allg(s) * (1.f / 64.f);
    float q = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = x1[t][e] - mean;
        xn[t][e] = d;
        q += d * d;
      }
    const float rstd = 1.f / sqrtf(m16_allg(q) * (1.f / 64.f) + a.eps);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const f32x4 gv = *reinterpret_cast<const f32x4*>(a.g2 + 16 * t + 4 * g);
      const f32x4 bv = *reinterpret_cast<const f32x4*>(a.b2n + 16 * t + 4 * g);
#pragma unroll
      for (int e = 0; e < 4; ++e) xn[t][e] = xn[t][e] * rstd * gv[e] + bv[e];
    }
  }
  FFN_STAMP(3);
  // ---- this wave's 128 hidden units: fc1 + GELU (8 tiles of 16), then its K-slice of fc2
  f32x4 hid[8];
  m16_gemm<8, 4, 4>(a.w1_f, 4, 8 * wave, 0, lane, hid, [&](int t, int r) { return xn[t][r]; });
  FFN_STAMP(4);
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const f32x4 bv = *reinterpret_cast<const f32x4*>(a.b1 + 128 * wave + 16 * t + 4 * g);
#pragma unroll
    for (int e = 0; e < 4; ++e) hid[t][e] = cmr_gelu(hid[t][e] + bv[e]);
  }
  FFN_STAMP(5);
  f32x4 part[4];
  m16_gemm<4, 8, 8>(a.w2_f, 64, 0, 8 * wave, lane, part, [&](int t, int r) { return hid[t][r]; });
  FFN_STAMP(6);
  if (wave > 0) {
#pragma unroll
    for (int t = 0; t < 4; ++t) *reinterpret_cast<f32x4*>(&red[(((wave - 1) * 4 + t) * 64 + lane) * 4]) = part[t];
  }
  __syncthreads();
  FFN_STAMP(7);
  if (wave != 0) return;
  f32x4 ov[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    f32x4 s = part[t];
#pragma unroll
    for (int w = 0; w < 7; ++w) s += *reinterpret_cast<const f32x4*>(&red[((w * 4 + t) * 64 + lane) * 4]);
    const f32x4 bv = *reinterpret_cast<const f32x4*>(a.b2 + 16 * t + 4 * g);
#pragma unroll
    for (int e = 0; e < 4; ++e) ov[t][e] = (s[e] + bv[e]) + x1[t][e];
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) cmr_pin(ov[t]);
  if (valid) {
    float* yp = a.out + (int64_t)row * a.ldo + 4 * g;
#pragma unroll
    for (int t = 0; t < 4; ++t) *reinterpret_cast<f32x4*>(yp + 16 * t) = ov[t];
  }
#ifdef CMR_FFN_STAMPS
  FFN_STAMP(8);
  if (lane == 0 && valid) {                            // debug build: the stage durations (100 MHz ticks of s_memtime) over the row's first floats
    float* yp = a.out + (int64_t)row * a.ldo;
    for (int i = 0; i < 8; ++i) yp[i] = (float)(st_[i + 1] - st_[i]);
    yp[8] = (float)(st_[0] & 0xffffff);
  }
#endif
}

}  // namespace

extern "C" int cmr_ln64_linear_f32(const float* x, int64_t ldx, int64_t rows_x, const float* wf_x, const float* bias_x,
                                   int n_out_x, float* out_x, int64_t ldo_x, const float* y, int64_t ldy, int64_t rows_y,
                                   const float* wf_y, const float* bias_y, int n_out_y, float* out_y, int64_t ldo_y,
                                   const float* gamma, const float* beta, float eps, hipStream_t stream) {
  CMR_REQUIRE(x && wf_x && bias_x && out_x && gamma && beta && rows_x > 0 && rows_x < (int64_t)0x7fffffc0);
  CMR_REQUIRE(n_out_x > 0 && n_out_x % 64 == 0 && ldx % 4 == 0 && ldo_x % 4 == 0 && cmr_aligned16(x) && cmr_aligned16(wf_x) &&
              cmr_aligned16(bias_x) && cmr_aligned16(out_x) && cmr_aligned16(gamma) && cmr_aligned16(beta));
  LnLinArgs a{};
  a.p[0] = LnLinProblem{x, ldx, (uint32_t)rows_x, wf_x, bias_x, n_out_x / 64, out_x, ldo_x};
  a.tiles0 = (uint32_t)((rows_x + 31) / 32);
  a.tiles = a.tiles0;
  if (y) {
    CMR_REQUIRE(wf_y && bias_y && out_y && rows_y > 0 && rows_y < (int64_t)0x7fffffc0 && n_out_y > 0 && n_out_y % 64 == 0);
    CMR_REQUIRE(ldy % 4 == 0 && ldo_y % 4 == 0 && cmr_aligned16(y) && cmr_aligned16(wf_y) && cmr_aligned16(bias_y) &&
                cmr_aligned16(out_y));
    a.p[1] = LnLinProblem{y, ldy, (uint32_t)rows_y, wf_y, bias_y, n_out_y / 64, out_y, ldo_y};
    a.tiles += (uint32_t)((rows_y + 31) / 32);
  } else {
    a.p[1] = a.p[0];
  }
  a.g = gamma; a.b = beta; a.eps = eps;
  // the proxy sets of this path are <= 169 tiles: one wave per workgroup spreads them over as many CUs (each wave's chain of L2
  // fragment loads then runs on its own CU) instead of packing four onto each of 43
  if (a.tiles <= 2048) hipLaunchKernelGGL(ln64_linear_kernel, dim3(a.tiles), dim3(64), 0, stream, a);
  else hipLaunchKernelGGL(ln64_linear_kernel, dim3((a.tiles + 3) / 4), dim3(256), 0, stream, a);
  return cmr_launch_status();
}

extern "C" int cmr_vit_out_ffn_f32(const float* ctx, int64_t ldc, const float* x, int64_t ldx, const float* wo_f,
                                   const float* bo, const float* ln_g, const float* ln_b, float eps, const float* w1_f,
                                   const float* b1, const float* w2_f, const float* b2, float* out, int64_t ldo, int64_t rows,
                                   hipStream_t stream) {
  CMR_REQUIRE(ctx && x && wo_f && bo && ln_g && ln_b && w1_f && b1 && w2_f && b2 && out && rows > 0 && rows < (int64_t)0x7fffffc0);
  CMR_REQUIRE(ldc % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && cmr_aligned16(ctx) && cmr_aligned16(x) && cmr_aligned16(out) &&
              cmr_aligned16(wo_f) && cmr_aligned16(w1_f) && cmr_aligned16(w2_f) && cmr_aligned16(bo) && cmr_aligned16(b1) &&
              cmr_aligned16(b2) && cmr_aligned16(ln_g) && cmr_aligned16(ln_b));
  const OutFfnArgs a{ctx, ldc, x, ldx, wo_f, bo, ln_g, ln_b, eps, w1_f, b1, w2_f, b2, out, ldo, (uint32_t)rows};
  hipLaunchKernelGGL(vit_out_ffn_kernel, dim3((unsigned)((rows + 31) / 32)), dim3(512), 0, stream, a);
  return cmr_launch_status();
}

extern "C" int cmr_vit_out_ffn16_f32(const float* ctx, int64_t ldc, const float* x, int64_t ldx, const float* wo_f16,
                                     const float* bo, const float* ln_g, const float* ln_b, float eps, const float* w1_f16,
                                     const float* b1, const float* w2_f16, const float* b2, float* out, int64_t ldo, int64_t rows,
                                     hipStream_t stream) {
  CMR_REQUIRE(ctx && x && wo_f16 && bo && ln_g && ln_b && w1_f16 && b1 && w2_f16 && b2 && out && rows > 0 && rows < (int64_t)0x7fffffe0);
  CMR_REQUIRE(ldc % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && cmr_aligned16(ctx) && cmr_aligned16(x) && cmr_aligned16(out) &&
              cmr_aligned16(wo_f16) && cmr_aligned16(w1_f16) && cmr_aligned16(w2_f16) && cmr_aligned16(bo) && cmr_aligned16(b1) &&
              cmr_aligned16(b2) && cmr_aligned16(ln_g) && cmr_aligned16(ln_b));
  const OutFfnArgs a{ctx, ldc, x, ldx, wo_f16, bo, ln_g, ln_b, eps, w1_f16, b1, w2_f16, b2, out, ldo, (uint32_t)rows};
  hipLaunchKernelGGL(vit_out_ffn16_kernel, dim3((unsigned)((rows + 15) / 16)), dim3(512), 0, stream, a);
  return cmr_launch_status();
}
