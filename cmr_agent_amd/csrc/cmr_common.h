// Shared device/host helpers for libcmr_hip.so (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define CMR_OK 0
#define CMR_EINVAL -1   // bad argument (shape / alignment / null pointer)
#define CMR_ELAUNCH -2  // hipGetLastError() after the launch was not hipSuccess
#define CMR_EUNSUPPORTED -3  // valid request that this build serves through another entry point (caller falls back)

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define CMR_REQUIRE(cond) \
  do {                    \
    if (!(cond)) return CMR_EINVAL; \
  } while (0)

static inline int cmr_launch_status() { return hipGetLastError() == hipSuccess ? CMR_OK : CMR_ELAUNCH; }

// Raises a kernel's dynamic-LDS limit (needed above 64 KB), once per (kernel, device): `cache` is a per-kernel array of
// the sizes already granted, indexed by device, so a process that drives several GPUs sets it on each of them.
constexpr int CMR_MAX_DEVICES = 16;
struct CmrSmemCache { size_t granted[CMR_MAX_DEVICES]; };
static inline int cmr_grant_smem(const void* kernel, size_t bytes, CmrSmemCache& cache) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return CMR_ELAUNCH;
  dev = dev < 0 || dev >= CMR_MAX_DEVICES ? 0 : dev;
  if (bytes <= 64 * 1024 || bytes <= cache.granted[dev]) return CMR_OK;
  if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return CMR_ELAUNCH;
  cache.granted[dev] = bytes;
  return CMR_OK;
}

static inline bool cmr_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// activation codes shared by the GEMM / conv epilogues
enum { CMR_ACT_NONE = 0, CMR_ACT_RELU = 1, CMR_ACT_LRELU = 2, CMR_ACT_GELU = 3, CMR_ACT_ELU1 = 4 };

// erf-GELU, v Phi(v) with Phi = 0.5 (1 + erf(v / sqrt 2)), and its derivative Phi(v) + v phi(v).  The ONE statement of both: the backward
// kernels recompute the forward's GELU from the saved pre-activation.  cmr_gelu_both gives the two from one erf (g has the bits of cmr_gelu:
// 0.5 v (1 + erf) is evaluated as written).
__device__ __forceinline__ float cmr_gelu(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f)); }
__device__ __forceinline__ float cmr_gelu_grad(float v) {
  return 0.5f * (1.f + erff(v * 0.70710678118654752440f)) + v * 0.39894228040143267794f * expf(-0.5f * v * v);
}
__device__ __forceinline__ void cmr_gelu_both(float v, float& g, float& dg) {
  const float e = 1.f + erff(v * 0.70710678118654752440f);
  g = 0.5f * v * e;
  dg = 0.5f * e + v * 0.39894228040143267794f * expf(-0.5f * v * v);
}

// exp(x) as v_exp_f32(x log2 e), and F.elu(v) + 1 on it -- libm's expf costs five more instructions per value for a range reduction that
// buys nothing at |v| of a projected feature (linear-attention state kernel 67 -> 62 us fp32, 39 -> 34 us bf16 at 8 x 26 752 rows)
__device__ __forceinline__ float cmr_exp2_fast(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }
__device__ __forceinline__ float cmr_elu1_fast(float v) { return v > 0.f ? v + 1.f : cmr_exp2_fast(v); }

__device__ __forceinline__ float cmr_act(float v, int act, float p) {
  switch (act) {
    case CMR_ACT_RELU: return v > 0.f ? v : 0.f;
    case CMR_ACT_LRELU: return v > 0.f ? v : v * p;
    case CMR_ACT_GELU: return cmr_gelu(v);
    case CMR_ACT_ELU1: return v > 0.f ? v + 1.f : expf(v);  // elu(v) + 1; libm's expf on purpose, not cmr_elu1_fast: full range and accuracy
    default: return v;
  }
}

// 32x32x2 fp32 MFMA: D[i][j] += sum_k A[i][k] B[k][j];  lane l supplies A[i=l&31][k=l>>5] and
// B[k=l>>5][j=l&31]; D register r of lane l is D[row=(r&3)+8*(r>>2)+4*(l>>5)][col=l&31].
// Pins a value in registers at this point of the program.  Epilogues compute every output first, pin it, and
// only then enter the predicated stores: hipcc otherwise sinks "acc + loaded operand" into each predicated
// block, where its waitcnt bookkeeping degrades to s_waitcnt vmcnt(0) -- every store then waits for the
// previous store (stores count in vmcnt on gfx9) and for the next tile's prefetch.
__device__ __forceinline__ void cmr_pin(f32x4& v) { asm volatile("" : "+v"(v)); }

__device__ __forceinline__ f32x16 cmr_mfma32(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// The value the partner lane (lane ^ 32) holds: v_permlane32_swap (gfx950) + a select, on the VALU -- __shfl_xor(v, 32) is a
// ds_bpermute_b32 round trip through LDS with an address and a wait (36 of them per tile in the linear-attention query layer).
// For 1-D workgroups whose size is a multiple of 64.
__device__ __forceinline__ float cmr_xhalf(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);      // r[0] = [lo | lo], r[1] = [hi | hi]
  return __builtin_bit_cast(float, (threadIdx.x & 32) ? r[0] : r[1]);
}

// LayerNorm over the 64 channels of a row of which this lane holds 32 and lane ^ 32 the other 32, in place; fp32 and bf16 twins share it.
// Two bodies by necessity, one per register layout, because their sums are ORDERED differently and every user's bits depend on the order:
//  * two MFMA accumulator tiles (register 4 qd + e of tile t = channel 32 t + 8 qd + 4 h + e): summed sequentially;
//  * eight float4 pieces, chan(i) = first channel of piece i: each piece summed pairwise, (v0 + v1) + (v2 + v3), then sequentially.
__device__ __forceinline__ void cmr_layernorm64(f32x16 (&v)[2], const float* __restrict__ gs, const float* __restrict__ bs, int h, float eps) {
  float s = 0.f;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) s += v[t][r];
  s += cmr_xhalf(s);
  const float mean = s * (1.f / 64.f);
  float q = 0.f;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float d = v[t][r] - mean;
      v[t][r] = d;
      q += d * d;
    }
  q += cmr_xhalf(q);
  const float rstd = 1.f / sqrtf(q * (1.f / 64.f) + eps);
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
      const f32x4 g = *reinterpret_cast<const f32x4*>(gs + 32 * t + 8 * qd + 4 * h);
      const f32x4 b = *reinterpret_cast<const f32x4*>(bs + 32 * t + 8 * qd + 4 * h);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[t][4 * qd + e] = v[t][4 * qd + e] * rstd * g[e] + b[e];
    }
}
template <typename CH>
__device__ __forceinline__ void cmr_layernorm64(f32x4 (&v)[8], const float* __restrict__ g, const float* __restrict__ b, float eps, CH chan) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
  s += cmr_xhalf(s);
  const float mean = s * (1.f / 64.f);
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = v[i][e] - mean;
      v[i][e] = d;
      q += d * d;
    }
  q += cmr_xhalf(q);
  const float rstd = 1.f / sqrtf(q * (1.f / 64.f) + eps);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const f32x4 gv = *reinterpret_cast<const f32x4*>(g + chan(i));
    const f32x4 bv = *reinterpret_cast<const f32x4*>(b + chan(i));
#pragma unroll
    for (int e = 0; e < 4; ++e) v[i][e] = v[i][e] * rstd * gv[e] + bv[e];
  }
}

// sum over a wave of doubles, the same value in every lane afterwards (fixed butterfly order: deterministic)
__device__ __forceinline__ double cmr_wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// fp32 -> bf16, round to nearest even (v_cvt_pk_bf16_f32): the ONE rounding of the bf16 kernels.  cmr_bf16_pack2 = bf16(lo) | bf16(hi) << 16.
// The two eight-wide packs give the same bits -- four v_cvt_pk_bf16_f32 each -- but NOT the same program: with `each` written as `pairs`,
// vit_fused_bf16.hip came out at 4752 instead of 4750 instruction lines with another register allocation and load order from the first tile
// on, and nobody has timed that.  Every kernel stays on the form it was written with; folding the two is a change to measure.
typedef __bf16 cmr_bf16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ unsigned cmr_bf16_pack2(float lo, float hi) {
  typedef float f2 __attribute__((ext_vector_type(2)));
  typedef __bf16 b2 __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(unsigned, __builtin_convertvector((f2){lo, hi}, b2));
}
__device__ __forceinline__ cmr_bf16x8 cmr_bf16x8_pairs(const f32x4& lo, const f32x4& hi) {       // four two-wide vector conversions
  return __builtin_bit_cast(cmr_bf16x8, uint4{cmr_bf16_pack2(lo[0], lo[1]), cmr_bf16_pack2(lo[2], lo[3]),
                                              cmr_bf16_pack2(hi[0], hi[1]), cmr_bf16_pack2(hi[2], hi[3])});
}
__device__ __forceinline__ cmr_bf16x8 cmr_bf16x8_each(const f32x4& lo, const f32x4& hi) {        // eight element casts
  cmr_bf16x8 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    r[i] = (__bf16)lo[i];
    r[4 + i] = (__bf16)hi[i];
  }
  return r;
}

// Maximum over the 32 lanes that share lane >> 5 (the 32 rows of a tile in the MFMA result layout), on the DPP data path: quad
// permutes, the two row mirrors and row_bcast:15 into rows 1 / 3 -- five VALU instructions per value and nothing through LDS
// (__shfl_xor compiles to ds_bpermute_b32: 160 LDS round trips + their waits per tile).  The result is valid in lanes 16..31 of
// each half.  max is exact and order independent: the same bits as before.
// (Done on the order-preserving integer image of the float -- k = bits ^ ((bits >> 31) & 0x7fffffff), an involution -- because a
// float max behind a DPP move is canonicalised first (two extra v_max per step) and is not folded into v_max_f32_dpp.)
template <int CTRL>
__device__ __forceinline__ int cmr_dpp(int v) { return __builtin_amdgcn_mov_dpp(v, CTRL, 0xf, 0xf, true); }      // every lane has a source
template <int CTRL, int ROWS>
__device__ __forceinline__ int cmr_dpp_rows(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, ROWS, 0xf, false); }
__device__ __forceinline__ int cmr_imax(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ float cmr_rowmax32(float x) {
  int m = __builtin_bit_cast(int, x);
  m ^= (m >> 31) & 0x7fffffff;
  m = cmr_imax(m, cmr_dpp<0xB1>(m));          // quad_perm:[1,0,3,2]
  m = cmr_imax(m, cmr_dpp<0x4E>(m));          // quad_perm:[2,3,0,1]
  m = cmr_imax(m, cmr_dpp<0x141>(m));         // row_half_mirror
  m = cmr_imax(m, cmr_dpp<0x140>(m));         // row_mirror
  m = cmr_imax(m, cmr_dpp_rows<0x142, 0xa>(m));    // row_bcast:15 -> rows 1 and 3 (rows 0 and 2 keep their own value)
  m ^= (m >> 31) & 0x7fffffff;
  return __builtin_bit_cast(float, m);
}

// Partner values for lane ^ 1 (DPP quad permute: folds into the consuming VALU instruction) and lane ^ 16 (v_permlane16_swap + select),
// instead of ds_bpermute_b32 round trips.  1-D workgroups, size a multiple of 64.
__device__ __forceinline__ float cmr_xor1(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, true));
}
__device__ __forceinline__ float cmr_xor16(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);      // r[0] = rows [0 0 2 2], r[1] = rows [1 1 3 3]
  return __builtin_bit_cast(float, (threadIdx.x & 16) ? r[0] : r[1]);
}

// The float on the same DPP move, and the sum over the 16 lanes of a DPP row as a butterfly (lane ^ 1, lane ^ 2, row_half_mirror,
// row_mirror), i.e. the balanced tree ((s0 + s1) + (s2 + s3)) + ...; IEEE addition commutes, so all 16 lanes hold the same bits.  Every
// lane of the wave must be active.  (guided_match.hip, pose_score.hip and visibility.hip; the matchers keep their own 16-lane cores.)
template <int CTRL>
__device__ __forceinline__ float cmr_fdpp(float v) { return __builtin_bit_cast(float, cmr_dpp<CTRL>(__builtin_bit_cast(int, v))); }
__device__ __forceinline__ float cmr_sum16(float s) {
  s += cmr_fdpp<0xB1>(s);           // quad_perm:[1,0,3,2]
  s += cmr_fdpp<0x4E>(s);           // quad_perm:[2,3,0,1]
  s += cmr_fdpp<0x141>(s);          // row_half_mirror
  s += cmr_fdpp<0x140>(s);          // row_mirror
  return s;
}

// Row selection: the caller's mask holds bytes (torch.bool / uint8) or 64-bit words (torch.int64); a row is selected where it is
// non-zero.  `mask` is never null here: an entry that accepts "no mask = every row" tests that at its call site (cmr_sel_or_all).
__device__ __forceinline__ bool cmr_sel(const void* mask, int mask_bytes, int64_t g) {
  return mask_bytes == 1 ? ((const uint8_t*)mask)[g] != 0 : ((const int64_t*)mask)[g] != 0;
}
__device__ __forceinline__ bool cmr_sel_or_all(const void* mask, int mask_bytes, int64_t g) {
  return !mask ? true : cmr_sel(mask, mask_bytes, g);
}

// The workgroup's number of set flags per flag, valid in every thread: ballot, popcount, one word per flag and wave in `part` (LDS).
// Integers: order free.  Every thread of the 1-D workgroup of THREADS calls it (it holds a barrier).
template <int NF, int THREADS>
__device__ __forceinline__ void cmr_block_counts(const bool (&flag)[NF], int (&part)[NF][THREADS / 64], int (&total)[NF]) {
  static_assert(THREADS == 256, "four waves");
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    const unsigned long long bal = __ballot(flag[f]);
    if ((threadIdx.x & 63) == 0) part[f][threadIdx.x >> 6] = __popcll(bal);
  }
  __syncthreads();
#pragma unroll
  for (int f = 0; f < NF; ++f) total[f] = part[f][0] + part[f][1] + part[f][2] + part[f][3];
}

// a * b + c with TWO roundings, and a + t (b - a) with three on top of it, so that plain fp32 torch code gives the same bits.  HIP's
// __fmul_rn / __fadd_rn are a plain product and sum that carry the translation unit's default -ffp-contract=fast, and the backend fuses
// them into one fma; plain operators under the pragma carry no such licence (and keep none after inlining).
__device__ __forceinline__ float cmr_mul_add_rn(float a, float b, float c) {
#pragma clang fp contract(off)
  const float m = a * b;
  return m + c;
}
__device__ __forceinline__ float cmr_lerp(float a, float b, float t) {
#pragma clang fp contract(off)
  const float d = b - a;
  return cmr_mul_add_rn(t, d, a);
}

// three finite coordinates: a row of a cloud that takes part
__device__ __forceinline__ bool cmr_finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// One Jacobi rotation that clears a[P][Q] of the symmetric N x N a in fp64 (N = 3: cloud_prepare.hip's covariance, N = 4: cloud_global.hip's
// quaternion matrix); v collects the rotations in its columns.  Sweep counts and sweep orders are the callers'.
template <int P, int Q, int N>
__device__ __forceinline__ void cmr_jacobi_rotate(double (&a)[N][N], double (&v)[N][N]) {
  const double apq = a[P][Q];
  if (apq == 0.0) return;
  const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
  const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));        // theta^2 = inf gives t = 0
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  a[P][P] -= t * apq;
  a[Q][Q] += t * apq;
  a[P][Q] = a[Q][P] = 0.0;
#pragma unroll
  for (int r = 0; r < N; ++r) {
    if (r == P || r == Q) continue;
    const double arp = a[r][P], arq = a[r][Q];
    a[r][P] = a[P][r] = c * arp - s * arq;
    a[r][Q] = a[Q][r] = s * arp + c * arq;
  }
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const double vp = v[k][P], vq = v[k][Q];
    v[k][P] = c * vp - s * vq;
    v[k][Q] = s * vp + c * vq;
  }
}

// ---- host helpers shared by the entries of the pose operations -------------------------------------------------------------------
// workspace sections start on 16 bytes
static inline int64_t cmr_up16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// a cloud of B x N rows against an h x w map: B is a grid's y extent, N / 256 its x extent, and a cell index must be exact in a float
static inline bool cmr_cloud_map_ok(int B, int N, int h, int w) {
  return B > 0 && B <= 65535 && N > 0 && (int64_t)N <= (int64_t)65535 * 256 && h > 0 && w > 0 && (int64_t)h * w <= (int64_t)1 << 24;
}

// workgroups of a fill kernel that writes `vecs` 16-byte vectors, one per thread; capped at 65536, the kernel strides beyond that
static inline unsigned cmr_fill_blocks(int64_t vecs, int threads) {
  const int64_t want = (vecs + threads - 1) / threads;
  return (unsigned)(want < 1 ? 1 : (want > 65536 ? 65536 : want));
}

// counts = 0 as a launch of its own, for an entry without a fill kernel to fold it into.  Internal to each source that launches it.
namespace {
template <int THREADS>
__global__ __launch_bounds__(THREADS) void cmr_zero_kernel(int32_t* __restrict__ counts, int ncounts) {
  for (int c = blockIdx.x * THREADS + threadIdx.x; c < ncounts; c += gridDim.x * THREADS) counts[c] = 0;
}
}  // namespace

__device__ __forceinline__ int cmr_mfma_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// Dropout mask, counter based (no state, no stored mask): element `idx` of dropout site `site` in the step whose seed is `seed` is KEPT
// iff the low 32 bits of a 64-bit mix (murmur3 finaliser) of the three reach thr = p * 2^32.  Forward and backward call it with the same
// arguments, so the backward pass regenerates the forward mask.  (seed, site) go through the finaliser FIRST and the element index is
// mixed into that key: with `(idx + site * G) ^ seed` in one mix, the mask of seed s + 1 was the mask of seed s with neighbouring
// elements swapped ((A ^ (s + 1)) == ((A ^ 1) ^ s) for even s), i.e. consecutive steps -- and ranks, whose seeds differ by a constant --
// dropped almost the same pattern.  The key is wave-uniform, so the second mix is the only per-element cost.
__device__ __forceinline__ uint64_t cmr_mix64(uint64_t x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}
__device__ __forceinline__ uint64_t cmr_drop_key(uint64_t seed, uint64_t site) { return cmr_mix64(seed + site * 0x9E3779B97F4A7C15ull); }
__device__ __forceinline__ bool cmr_keep(uint64_t seed, uint64_t site, uint64_t idx, uint32_t thr) {
  return (uint32_t)cmr_mix64(cmr_drop_key(seed, site) ^ idx) >= thr;
}
// one dropout site with the wave-uniform half of cmr_keep hoisted: mul(idx) = the 1 / (1 - p) scale where element idx is kept, else 0
struct CmrDrop {
  uint64_t key;
  uint32_t thr;
  float scale;
  __device__ __forceinline__ void init(const int64_t* seed, uint64_t site, uint32_t thr_, float scale_) {
    key = cmr_drop_key((uint64_t)seed[0], site);
    thr = thr_;
    scale = scale_;
  }
  __device__ __forceinline__ float mul(uint64_t idx) const { return (uint32_t)cmr_mix64(key ^ idx) >= thr ? scale : 0.f; }
};
static inline uint32_t cmr_drop_threshold(float p) {
  const double t = (double)p * 4294967296.0;
  return t <= 0.0 ? 0u : (t >= 4294967295.0 ? 4294967295u : (uint32_t)t);
}

