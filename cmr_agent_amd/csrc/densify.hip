// Image-guided densification of a sparse depth / attribute map (port extension): the joint bilateral filter as a
// normalised convolution.  A pixel of depth is a SAMPLE iff it is finite and > 0 (ops.render_points / ops.visibility write +inf where no
// row landed); every pixel takes the weighted mean of the samples of its (2R + 1)^2 window, weights falling with distance and with the
// difference of the guide image's colours.
//
// cmr_densify_f32 -- two launches on the caller's stream, no workspace:
//   cmr_zero_kernel    counts = 0 (cmr_common.h).
//   dn_densify_kernel  one 256-thread workgroup per DN_TW x DN_TH = 64 x 16 tile on (ceil(w / 64) ceil(h / 16), B); templated on the
//                      number of guide planes and on "has attributes".
//     stage   the depth tile with its halo of R pixels ((16 + 2R) x (64 + 2R) floats) and the guide planes go to LDS once, one
//             coalesced 64-float line per wave and step; outside the map and on non-samples the depth is 0.  The same step leaves a
//             VALIDITY BITMAP: __ballot of "is a sample", two 64-bit words per halo line.
//     gather  thread (x = t & 63, t >> 6) owns the four pixels (x, 4 (t >> 6) + i).  For every line of the window it cuts its
//             2R + 1 bits out of the line's bitmap (a broadcast LDS read and two shifts) and walks the SET bits only, lowest first
//             (ctz, clear): 85 - 98 % of the taps are empty and cost nothing but their share of the mask.  A wave walks as long as
//             its busiest lane, about 3 steps a line at 4 % density instead of 2R + 1.  Per sample: dx^2 + dy^2 is an exact
//             integer, the guide term a chain of fmas, and ONE v_exp_f32 takes -(t ks + s kr) with log2 e folded into ks and kr
//             on the host (in double).  A pixel's sums run line by line, left to right: the order is fixed, no floating-point
//             atomic exists, so two calls agree bit for bit and a sample's result depends on its own maps only.
//             Attributes are read at samples only, from global memory (the taps of neighbouring pixels hit the same lines).
//     counts  (samples in the map, pixels with n > 0, filled pixels): a wave reduction of each thread's three integers, one integer
//             atomic per workgroup and word.
// LDS: (1 + Cg) (16 + 2R) (64 + 2R) 4 + (16 + 2R) 16 bytes, dynamic: 10.8 KB at R = 8 without a guide, 41.5 KB with 3 planes, 92 928 B
// at R = 16 with 4 (one workgroup per CU; granted through cmr_grant_smem).
#include "cmr_project.h"   // CMR_MAX_RADIUS

namespace {

constexpr int DN_THREADS = 256;
constexpr int DN_TW = 64;          // tile width = one wave per tile line
constexpr int DN_TH = 16;          // tile height: 4 waves x DN_PPT lines
constexpr int DN_PPT = DN_TH / (DN_THREADS / 64);
constexpr int DN_MAX_C = 4;

struct DnParams {
  const float* depth;
  const float* guide;
  const float* attr;
  float* dense_depth;
  float* dense_attr;
  float* conf;
  int32_t* count;
  int32_t* counts;
  int C, h, w, R, keep;
  float ks, kr;        // log2 e / (2 sigma_s^2), log2 e / (2 sigma_r^2)
  float min_weight, fill;
};

template <int CG, bool ATTR>
__global__ __launch_bounds__(DN_THREADS) void dn_densify_kernel(const DnParams p) {
  extern __shared__ __align__(16) unsigned char dn_smem[];
  __shared__ int part[3][DN_THREADS / 64];
  const int R = p.R, h = p.h, w = p.w;
  const int LW = DN_TW + 2 * R, LH = DN_TH + 2 * R, LP = LW * LH;
  unsigned long long* bits = reinterpret_cast<unsigned long long*>(dn_smem);             // [LH][2]
  float* sd = reinterpret_cast<float*>(dn_smem + (size_t)LH * 16);                       // [LH][LW]
  float* sg = sd + LP;                                                                   // [CG][LH][LW]
  const int tiles_x = (w + DN_TW - 1) / DN_TW, tile_y = blockIdx.x / tiles_x;            // tiles ride in gridDim.x: up to 2^20 lines of them
  const int b = blockIdx.y, x0 = (blockIdx.x - tile_y * tiles_x) * DN_TW, y0 = tile_y * DN_TH;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t cells = (int64_t)h * w;
  const float* db = p.depth + (int64_t)b * cells;
  const float* gb = CG ? p.guide + (int64_t)b * CG * cells : nullptr;

  // stage: wave-uniform (line, half) steps; every address is tested against the map before it is read
  for (int s = wave; s < 2 * LH; s += DN_THREADS / 64) {
    const int lr = s >> 1, lc = (s & 1) * 64 + lane;
    const int gy = y0 - R + lr, gx = x0 - R + lc;
    const bool inmap = lc < LW && gy >= 0 && gy < h && gx >= 0 && gx < w;
    const int g = inmap ? gy * w + gx : 0;
    float z = inmap ? db[g] : 0.f;
    float gv[CG ? CG : 1];
#pragma unroll
    for (int c = 0; c < CG; ++c) gv[c] = inmap ? gb[(int64_t)c * cells + g] : 0.f;
    const bool sample = z > 0.f && z < __builtin_huge_valf();                             // false for NaN, 0, negatives and both infinities
    z = sample ? z : 0.f;
    const unsigned long long bal = __ballot(sample);
    if (lane == 0) bits[s] = bal;
    if (lc < LW) {
      sd[lr * LW + lc] = z;
#pragma unroll
      for (int c = 0; c < CG; ++c) sg[c * LP + lr * LW + lc] = gv[c];
    }
  }
  __syncthreads();

  const unsigned long long wmask = (1ull << (2 * R + 1)) - 1ull;                          // 2R + 1 <= 33 bits
  const int gx = x0 + lane;
  int n_sample = 0, n_any = 0, n_filled = 0;
  for (int i = 0; i < DN_PPT; ++i) {
    const int ly = wave * DN_PPT + i, gy = y0 + ly;                                       // wave-uniform
    if (gy >= h) break;
    if (gx >= w) continue;
    const int pc = (ly + R) * LW + lane + R;                                              // the pixel itself in the halo tile
    float gp[CG ? CG : 1];
#pragma unroll
    for (int c = 0; c < CG; ++c) gp[c] = sg[c * LP + pc];
    float S0 = 0.f, S1 = 0.f, A[DN_MAX_C] = {0.f, 0.f, 0.f, 0.f};
    int n = 0;
    for (int r = 0; r <= 2 * R; ++r) {
      const int lr = ly + r;
      const unsigned long long lo = bits[2 * lr], hi = bits[2 * lr + 1];
      unsigned long long m = lo >> lane;
      if (lane) m |= hi << (64 - lane);
      m &= wmask;
      n += __popcll(m);
      const int dy = r - R, dy2 = dy * dy;
      const int rowbase = lr * LW + lane;
      while (m) {
        const int j = __builtin_ctzll(m);
        m &= m - 1ull;
        const int q = rowbase + j, dx = j - R;
        const float z = sd[q];
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < CG; ++c) {
          const float d = gp[c] - sg[c * LP + q];
          s = c ? fmaf(d, d, s) : d * d;
        }
        const float t = (float)(dx * dx + dy2);                                           // exact: <= 512
        const float a = CG ? fmaf(s, p.kr, t * p.ks) : t * p.ks;
        const float wt = __builtin_amdgcn_exp2f(-a);                                      // weights below 2^-126 count as 0
        S0 += wt;
        S1 = fmaf(wt, z, S1);
        if (ATTR) {
          const float* ab = p.attr + (int64_t)b * p.C * cells + ((gy + dy) * w + gx + dx);
#pragma unroll
          for (int k = 0; k < DN_MAX_C; ++k) A[k] = fmaf(wt, ab[(int64_t)(k < p.C ? k : p.C - 1) * cells], A[k]);
        }
      }
    }
    const float own = sd[pc];
    const bool is_sample = own > 0.f;
    const bool filled = S0 >= p.min_weight;
    const bool kept = p.keep && is_sample;
    const int g = gy * w + gx;
    const int64_t o = (int64_t)b * cells + g;
    p.dense_depth[o] = kept ? own : (filled ? S1 / S0 : __builtin_huge_valf());
    p.conf[o] = S0;
    if (p.count) p.count[o] = n;
    if (ATTR) {
      const float* ab = p.attr + (int64_t)b * p.C * cells + g;
      float* ob = p.dense_attr + (int64_t)b * p.C * cells + g;
#pragma unroll
      for (int k = 0; k < DN_MAX_C; ++k)
        if (k < p.C) ob[(int64_t)k * cells] = kept ? ab[(int64_t)k * cells] : (filled ? A[k] / S0 : p.fill);
    }
    n_sample += is_sample;
    n_any += n > 0;
    n_filled += filled;
  }
  // every thread arrives here: the loops above hold no barrier
  int v[3] = {n_sample, n_any, n_filled};
#pragma unroll
  for (int f = 0; f < 3; ++f) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v[f] += __shfl_xor(v[f], off);
    if (lane == 0) part[f][wave] = v[f];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int tot = part[threadIdx.x][0] + part[threadIdx.x][1] + part[threadIdx.x][2] + part[threadIdx.x][3];
    if (tot) atomicAdd(&p.counts[3 * b + threadIdx.x], tot);
  }
}

inline size_t dn_smem_bytes(int R, int cg) {
  const size_t LW = DN_TW + 2 * R, LH = DN_TH + 2 * R;
  return LH * 16 + (size_t)(1 + cg) * LW * LH * sizeof(float);
}

template <int CG, bool ATTR>
int dn_launch(const DnParams& p, int B, hipStream_t stream) {
  const size_t smem = dn_smem_bytes(p.R, CG);
  static CmrSmemCache granted{};
  if (cmr_grant_smem(reinterpret_cast<const void*>(dn_densify_kernel<CG, ATTR>), smem, granted) != CMR_OK) return CMR_ELAUNCH;
  const dim3 grid(((p.w + DN_TW - 1) / DN_TW) * ((p.h + DN_TH - 1) / DN_TH), B);
  hipLaunchKernelGGL((dn_densify_kernel<CG, ATTR>), grid, dim3(DN_THREADS), smem, stream, p);
  return cmr_launch_status();
}

template <bool ATTR>
int dn_dispatch(const DnParams& p, int Cg, int B, hipStream_t stream) {
  switch (Cg) {
    case 0: return dn_launch<0, ATTR>(p, B, stream);
    case 1: return dn_launch<1, ATTR>(p, B, stream);
    case 2: return dn_launch<2, ATTR>(p, B, stream);
    case 3: return dn_launch<3, ATTR>(p, B, stream);
    default: return dn_launch<4, ATTR>(p, B, stream);
  }
}

}  // namespace

extern "C" int cmr_densify_f32(const float* depth, const float* attr, int C, const float* guide, int Cg, int B, int h, int w, int radius,
                               float sigma_s, float sigma_r, float min_weight, int keep, float fill, float* dense_depth, float* dense_attr,
                               float* conf, int32_t* count, int32_t* counts, hipStream_t stream) {
  CMR_REQUIRE(depth && dense_depth && conf && counts);
  CMR_REQUIRE(B > 0 && B <= 65535 && h > 0 && w > 0 && (int64_t)h * w <= (int64_t)1 << 24);
  CMR_REQUIRE((attr == nullptr) == (dense_attr == nullptr) && (attr ? (C >= 1 && C <= DN_MAX_C) : C == 0));
  CMR_REQUIRE(guide ? (Cg >= 1 && Cg <= DN_MAX_C) : Cg == 0);
  CMR_REQUIRE(radius >= 0 && radius <= CMR_MAX_RADIUS && (keep == 0 || keep == 1));
  CMR_REQUIRE(sigma_s > 0.f && sigma_s < __builtin_huge_valf() && min_weight >= 1e-24f && min_weight < __builtin_huge_valf());
  CMR_REQUIRE(!guide || (sigma_r > 0.f && sigma_r < __builtin_huge_valf()));
  const double log2e = 1.4426950408889634074;
  DnParams p;
  p.depth = depth; p.guide = guide; p.attr = attr;
  p.dense_depth = dense_depth; p.dense_attr = dense_attr; p.conf = conf; p.count = count; p.counts = counts;
  p.C = C; p.h = h; p.w = w; p.R = radius; p.keep = keep;
  p.ks = (float)(log2e / (2.0 * (double)sigma_s * (double)sigma_s));                     // one rounding each
  p.kr = guide ? (float)(log2e / (2.0 * (double)sigma_r * (double)sigma_r)) : 0.f;
  p.min_weight = min_weight; p.fill = fill;
  CMR_REQUIRE(p.ks < __builtin_huge_valf() && p.kr < __builtin_huge_valf());
  hipLaunchKernelGGL(cmr_zero_kernel<DN_THREADS>, dim3(1), dim3(DN_THREADS), 0, stream, counts, 3 * B);
  return attr ? dn_dispatch<true>(p, Cg, B, stream) : dn_dispatch<false>(p, Cg, B, stream);
}
