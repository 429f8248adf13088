// Dual-softmax match confidence ahead of PnP-RANSAC (port extension): the nearest pixel feature of every selected point as
// cmr_feat_match_f32 finds it, and for that match the product of its probability under a softmax over the point's row and under a
// softmax over the pixel's column of the similarity matrix s(n, p) = -d^2(n, p) / T (the selected points x the sample's pixels):
//   conf[n] = exp(2 s(n, idx[n]) - row_lse[n] - col_lse[idx[n]]).
//
// Launches, all enqueued on the caller's stream:
//   mc_count_kernel / mc_pack_kernel  selected rows of every sample -> a row list in ROW ORDER (two-pass count + scan, no atomics);
//   mc_sweep_kernel<MC_FWD>   queries = listed points, streamed = the sample's pixels: fm_match_kernel's tile shape and arithmetic
//                             (|q|^2 - 2 p.q on 32x32x2 fp32 MFMA, pixels = A rows from LDS tiles of 64, queries = B columns in registers,
//                             strict < in increasing pixel order), so idx is cmr_feat_match_f32's idx bit for bit -- and beside the running
//                             (min, index) an online log-sum-exp in base 2: the running minimum v_min of the score v = |q|^2 - 2 p.q is,
//                             up to the query's own |x|^2 and the factor k = log2(e) / T, the running maximum of s, so after the 16
//                             scores of a 32-pixel sub-tile a lane rescales its sum by exp2(k v_min_new - k v_min_old) and adds
//                             exp2(k v_min - k v) for each of them (one fma, one v_exp_f32, one add per score);
//   mc_sweep_kernel<MC_REV>   the same problem with the roles swapped: queries = pixels, streamed = the listed points (gathered through
//                             the list in row order); the running minimum carries no index;
//   mc_col_kernel             folds the reverse ranges (below) into col_lse, one thread per pixel;
//   mc_final_kernel           one thread per row: folds the forward ranges into idx, d1, row_lse, gathers col_lse[idx], writes conf, keep
//                             and the unselected rows' fill values, and counts (reduced per workgroup through LDS, at most one integer
//                             atomic per word and workgroup).
// Splits: a sweep cuts the STREAMED side into up to MC_SPLITS contiguous ranges of tiles (gridDim.z); each workgroup writes its range's
// (minimum, index, sum relative to that minimum) to a slot of its own and the fold takes them in range order: the minimum with the same
// strict <, the sum as sum_z S_z exp2(k min - k min_z).  Where the ranges are cut changes the rounding of that sum, so the cut is a
// function of the sample's own selected count and the map size ONLY (never of B): a sample's outputs are the same bits alone and inside
// any batch.  Every result is a plain store from the one workgroup / thread that owns it: no floating-point atomics, no launch-order
// dependence.
#include "cmr_common.h"

namespace {

constexpr int MC_C = 64;          // feature width (the model's only one)
constexpr int MC_THREADS = 256;   // 4 waves
constexpr int MC_ROWS = 256;      // queries per workgroup: wave w holds queries 64w .. 64w+63 as two 32-column B tiles
constexpr int MC_TILE = 64;       // streamed rows per LDS tile: 64 rows of 16 float4 chunks, chunk c of row r stored at c ^ (r & 15)
constexpr int MC_CHUNK = 256;     // rows per compaction workgroup
constexpr int MC_SPLITS = 8;      // most ranges the streamed side of a sweep is cut into
constexpr int MC_TARGET = 1024;   // workgroups per sample a sweep aims for
constexpr float MC_KCAP = 1e30f;  // the scaled minimum k * v_min of a lane that has seen no streamed row yet (finite: no inf - inf)

enum { MC_FWD = 0, MC_REV = 1 };

__device__ __forceinline__ unsigned mc_xhalf_u(unsigned u) {
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return (threadIdx.x & 32) ? r[0] : r[1];
}

// v_exp_f32: base 2, no denormal results (an argument under -126 gives 0, which is what a term that small is worth here)
__device__ __forceinline__ float mc_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// the softmax's running maximum in base 2, from the running minimum of the score (monotone, so the minimum of the scaled values is the
// scaled minimum: sweep and folds recompute it from the stored minimum instead of storing it)
__device__ __forceinline__ float mc_kmin(float kscale, float vmin) { return fminf(MC_KCAP, kscale * vmin); }

// ---- order-preserving compaction ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MC_CHUNK) void mc_count_kernel(const void* __restrict__ mask, int mask_bytes, int N, int nchunk,
                                                            int32_t* __restrict__ chunk_cnt) {
  __shared__ int wc[MC_CHUNK / 64];
  const int b = blockIdx.y, n = blockIdx.x * MC_CHUNK + threadIdx.x;
  const bool sel = n < N && cmr_sel(mask, mask_bytes, (int64_t)b * N + n);
  const int c = __popcll(__ballot(sel));
  if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) chunk_cnt[(int64_t)b * nchunk + blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

__global__ __launch_bounds__(MC_CHUNK) void mc_pack_kernel(const void* __restrict__ mask, int mask_bytes, int N, int nchunk,
                                                           const int32_t* __restrict__ chunk_cnt, int32_t* __restrict__ list,
                                                           int32_t* __restrict__ counts) {
  __shared__ int red[MC_CHUNK];
  __shared__ int wc[MC_CHUNK / 64];
  const int b = blockIdx.y, c = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int s = 0;
  for (int i = threadIdx.x; i < c; i += MC_CHUNK) s += chunk_cnt[(int64_t)b * nchunk + i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int k = MC_CHUNK / 2; k > 0; k >>= 1) {
    if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  const int base = red[0];
  const int n = c * MC_CHUNK + threadIdx.x;
  const bool sel = n < N && cmr_sel(mask, mask_bytes, (int64_t)b * N + n);
  const unsigned long long bal = __ballot(sel);
  if (lane == 0) wc[wave] = __popcll(bal);
  __syncthreads();
  int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) pos += wc[w];
  if (sel) list[(int64_t)b * N + pos] = n;
  if (c == nchunk - 1 && threadIdx.x == 0) counts[4 * b] = base + wc[0] + wc[1] + wc[2] + wc[3];   // = the number of selected rows
}

// ---- the sweeps ----------------------------------------------------------------------------------------------------------------------
// Stages streamed rows [j0, j0 + 64) of one sample: thread t loads a quarter row (4 float4) of row t >> 2 into registers.  Forward the
// rows are the pixels themselves, in the reverse sweep the listed points.
template <int MODE>
__device__ __forceinline__ void mc_load(const float* __restrict__ pc_b, const float* __restrict__ img_b, const int32_t* __restrict__ list_b,
                                        int ns, int j0, float4 (&v)[4]) {
  const int j = j0 + (threadIdx.x >> 2);
  if (j < ns) {
    const float* row = MODE == MC_REV ? pc_b + (int64_t)list_b[j] * MC_C : img_b + (int64_t)j * MC_C;
    const float4* src = reinterpret_cast<const float4*>(row) + 4 * (threadIdx.x & 3);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = src[i];
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// ... and writes them (swizzled) plus the row's squared norm; rows past the end get +inf: never chosen, and a term of exactly 0.
__device__ __forceinline__ void mc_store(float4* tile, float* qn, int ns, int j0, const float4 (&v)[4]) {
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
  if (q == 0) qn[r] = j0 + r < ns ? s : __builtin_huge_valf();
}

// How a sweep with nq queries and ns streamed rows in ONE sample is cut: -> the number of ranges in use (<= MC_SPLITS), tps = tiles per
// range.  A function of the sample's own two sizes only; sweep and fold call it with the same arguments.
__device__ __forceinline__ int mc_splits(int nq, int ns, int& tps) {
  const int ntile = (ns + MC_TILE - 1) / MC_TILE;
  tps = 0;
  if (ntile == 0 || nq == 0) return 0;
  const int qwg = (nq + MC_ROWS - 1) / MC_ROWS;
  int want = (MC_TARGET + qwg - 1) / qwg;
  want = want < MC_SPLITS ? want : MC_SPLITS;
  want = want < ntile ? want : ntile;
  want = want > 1 ? want : 1;
  tps = (ntile + want - 1) / want;
  return (ntile + tps - 1) / tps;
}

template <int MODE>
__global__ __launch_bounds__(256) void mc_sweep_kernel(const float* __restrict__ pc, const float* __restrict__ img, const int32_t* __restrict__ list,
                                                       int N, int hw, float kscale, const int32_t* __restrict__ counts,
                                                       float* __restrict__ norm, float* __restrict__ pv, int32_t* __restrict__ pi,
                                                       float* __restrict__ ps, int64_t pstride) {
  __shared__ float4 tile[2][MC_TILE * 16];
  __shared__ __attribute__((aligned(16))) float qn[2][MC_TILE];
  const int b = blockIdx.y;
  const int nsel = counts[4 * b];                                   // written by mc_pack_kernel (an earlier launch on the stream)
  const int nq = MODE == MC_REV ? hw : nsel;                        // queries (B columns, registers)
  const int ns = MODE == MC_REV ? nsel : hw;                        // streamed rows (A rows, LDS)
  const int row0 = blockIdx.x * MC_ROWS;
  if (row0 >= nq) return;
  int tps;
  const int nact = mc_splits(nq, ns, tps);
  if ((int)blockIdx.z >= nact) return;
  const int ntile = (ns + MC_TILE - 1) / MC_TILE;
  const int t_begin = blockIdx.z * tps;
  const int t_end = t_begin + tps < ntile ? t_begin + tps : ntile;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int half = lane >> 5, col = lane & 31;
  const float* img_b = img + (int64_t)b * hw * MC_C;
  const float* pc_b = pc + (int64_t)b * N * MC_C;
  const int32_t* list_b = list + (int64_t)b * N;
  const int64_t qbase = MODE == MC_REV ? (int64_t)b * hw : (int64_t)b * N;

  // B operand: lane holds features 32*half .. 32*half+31 of its column's query (k of MFMA step s is 32*half + s, on both operands)
  float bq[2][32];
  int n_of[2];                                                      // forward: the query's row number n; reverse: its pixel
  bool valid[2];
  float pn[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int r = row0 + 64 * wave + 32 * t + col;
    valid[t] = r < nq;
    n_of[t] = valid[t] ? (MODE == MC_REV ? r : list_b[r]) : 0;
    const float* row = MODE == MC_REV ? img_b + (int64_t)n_of[t] * MC_C : pc_b + (int64_t)n_of[t] * MC_C;
    const float4* src = reinterpret_cast<const float4*>(row + 32 * half);
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
  int bidx[2] = {t_begin * MC_TILE, t_begin * MC_TILE};             // all-NaN scores keep the range's first entry, as torch.argmin
  float km[2] = {MC_KCAP, MC_KCAP};                                 // = mc_kmin(kscale, best) after every sub-tile
  float sum[2] = {0.f, 0.f};                                        // sum of exp2(km - k v) over the streamed rows this lane has seen
  const float nk = -kscale;
  float4 pre[4];
  mc_load<MODE>(pc_b, img_b, list_b, ns, t_begin * MC_TILE, pre);
  mc_store(tile[0], qn[0], ns, t_begin * MC_TILE, pre);
  __syncthreads();
  for (int it = t_begin; it < t_end; ++it) {
    const int buf = (it - t_begin) & 1, p0 = it * MC_TILE;
    const bool more = it + 1 < t_end;
    if (more) mc_load<MODE>(pc_b, img_b, list_b, ns, p0 + MC_TILE, pre);
#pragma unroll 1
    for (int u = 0; u < 2; ++u) {                                   // two 32-row sub-tiles
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
      float v0[16], v1[16];
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int o = 32 * u + 8 * g4 + 4 * half;
        const float4 q4 = *reinterpret_cast<const float4*>(&qn[buf][o]);
        const float qv[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int g = 4 * g4 + e;
          const int pix = p0 + o + e;                               // = cmr_mfma_row(g, lane): increasing with g in a lane
          v0[g] = fmaf(-2.f, acc0[g], qv[e]);
          v1[g] = fmaf(-2.f, acc1[g], qv[e]);
          if (MODE == MC_REV) {
            best[0] = fminf(best[0], v0[g]);
            best[1] = fminf(best[1], v1[g]);
          } else {
            if (v0[g] < best[0]) { best[0] = v0[g]; bidx[0] = pix; }  // strict: the first (lowest) entry of a tie stays
            if (v1[g] < best[1]) { best[1] = v1[g]; bidx[1] = pix; }
          }
        }
      }
      // online log-sum-exp: move the sum to the new minimum (exp2(0) = 1 when it did not move), then the 16 terms, each <= 1
      const float k0 = mc_kmin(kscale, best[0]), k1 = mc_kmin(kscale, best[1]);
      float s0 = sum[0] * mc_exp2(k0 - km[0]), s1 = sum[1] * mc_exp2(k1 - km[1]);
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        s0 += mc_exp2(fmaf(nk, v0[g], k0));
        s1 += mc_exp2(fmaf(nk, v1[g], k1));
      }
      sum[0] = s0; sum[1] = s1; km[0] = k0; km[1] = k1;
    }
    if (more) mc_store(tile[buf ^ 1], qn[buf ^ 1], ns, p0 + MC_TILE, pre);
    __syncthreads();
  }

  // the two lane halves saw interleaved streamed rows: lower score wins, a tie goes to the lower index; the sums meet at the joint minimum
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const float ob = __builtin_bit_cast(float, mc_xhalf_u(__builtin_bit_cast(unsigned, best[t])));
    const int oi = (int)mc_xhalf_u((unsigned)bidx[t]);
    const float os = __builtin_bit_cast(float, mc_xhalf_u(__builtin_bit_cast(unsigned, sum[t])));
    const float okm = mc_kmin(kscale, ob);
    if (ob < best[t] || (ob == best[t] && oi < bidx[t])) { best[t] = ob; bidx[t] = oi; }
    const float kj = mc_kmin(kscale, best[t]);
    const float tot = sum[t] * mc_exp2(kj - km[t]) + os * mc_exp2(kj - okm);     // half 0 stores: its own sum first
    if (!(valid[t] && half == 0)) continue;
    const int64_t slot = blockIdx.z * pstride + qbase + n_of[t];
    pv[slot] = best[t];
    ps[slot] = tot;
    if (MODE == MC_FWD) pi[slot] = bidx[t];
    if (blockIdx.z == 0) norm[qbase + n_of[t]] = pn[t];
  }
}

// ---- folds ---------------------------------------------------------------------------------------------------------------------------
// The ranges of one query in range order: -> the minimum (strict <: the lowest index of a tie stays), its index (pi may be null) and the
// sum of exp2(k min - k v) over everything streamed.
__device__ __forceinline__ void mc_fold(const float* __restrict__ pv, const int32_t* __restrict__ pi, const float* __restrict__ ps,
                                        int64_t pstride, int64_t g, int nact, float kscale, float& best, int& p, float& tot) {
  best = pv[g];
  p = pi ? pi[g] : 0;
  for (int z = 1; z < nact; ++z) {
    const float v = pv[z * pstride + g];
    if (v < best) { best = v; if (pi) p = pi[z * pstride + g]; }
  }
  const float kj = mc_kmin(kscale, best);
  tot = 0.f;
  for (int z = 0; z < nact; ++z) tot += ps[z * pstride + g] * exp2f(kj - mc_kmin(kscale, pv[z * pstride + g]));
}

// col_lse of every pixel from the reverse ranges, the listed points in row order; -inf when nothing is selected.
__global__ __launch_bounds__(256) void mc_col_kernel(int hw, float kscale, float temp, const int32_t* __restrict__ counts,
                                                     const float* __restrict__ qnorm, const float* __restrict__ pv,
                                                     const float* __restrict__ ps, int64_t pstride, float* __restrict__ col) {
  const int b = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
  if (p >= hw) return;
  const int64_t g = (int64_t)b * hw + p;
  int tps;
  const int nact = mc_splits(hw, counts[4 * b], tps);
  float lse = -__builtin_huge_valf();
  if (nact > 0) {
    float best, tot;
    int unused;
    mc_fold(pv, nullptr, ps, pstride, g, nact, kscale, best, unused, tot);
    lse = logf(tot) - (qnorm[g] + best) / temp;                  // log sum_n exp(-d^2 / T), d^2 of the nearest point = |q|^2 + min
  }
  col[g] = lse;
}

// ---- idx, d1, row_lse, conf, keep + counts -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mc_final_kernel(const void* __restrict__ mask, int mask_bytes, int N, int hw, int w, float kscale,
                                                       float temp, float min_conf, const float* __restrict__ gt_xy, float thr,
                                                       const float* __restrict__ pnorm, const float* __restrict__ pv,
                                                       const int32_t* __restrict__ pi, const float* __restrict__ ps, int64_t pstride,
                                                       const float* __restrict__ col, int32_t* __restrict__ idx, float* __restrict__ conf,
                                                       uint8_t* __restrict__ keep, float* __restrict__ d1, float* __restrict__ row_lse,
                                                       int32_t* __restrict__ counts) {
  __shared__ int part[256 / 64][4];
  const int b = blockIdx.y;
  const int n = blockIdx.x * 256 + threadIdx.x;
  const int64_t g = (int64_t)b * N + n;
  const int nsel = counts[4 * b];                                   // this kernel adds to the other three entries only
  bool kept = false, inl = false;
  if (n < N) {
    const float nanv = __builtin_nanf("");
    int p = -1;
    float c = nanv, dist = nanv, lse = nanv;
    if (cmr_sel(mask, mask_bytes, g)) {
      int tps;
      const int nact = mc_splits(nsel, hw, tps);
      float best, tot;
      mc_fold(pv, pi, ps, pstride, g, nact, kscale, best, p, tot);
      const float d2 = pnorm[g] + best;
      const float s = -d2 / temp, lt = logf(tot);                  // row_lse = s + log(sum of exp(s' - s)), the sum >= its own term 1
      lse = s + lt;
      dist = sqrtf(fmaxf(d2, 0.f));
      c = fminf(1.f, expf((s - lt) - col[(int64_t)b * hw + p]));    // 2 s - row_lse - col_lse
      kept = !(min_conf > 0.f) || c >= min_conf;
      if (gt_xy) {
        const float x = gt_xy[(int64_t)b * 2 * N + n], y = gt_xy[(int64_t)b * 2 * N + N + n];
        const float dx = (float)(p % w) - x, dy = (float)(p / w) - y;
        inl = isfinite(x) && isfinite(y) && sqrtf(dx * dx + dy * dy) <= thr;
      }
    }
    idx[g] = p;
    conf[g] = c;
    keep[g] = kept ? 1 : 0;
    if (d1) d1[g] = dist;
    if (row_lse) row_lse[g] = lse;
  }
  const int c1 = __popcll(__ballot(kept)), c2 = __popcll(__ballot(kept && inl)), c3 = __popcll(__ballot(inl));
  if ((threadIdx.x & 63) == 0) {
    int* q = part[threadIdx.x >> 6];
    q[1] = c1; q[2] = c2; q[3] = c3;
  }
  __syncthreads();
  if (threadIdx.x >= 1 && threadIdx.x < 4) {
    const int t = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
    if (t) atomicAdd(&counts[4 * b + threadIdx.x], t);
  }
}

struct McWorkspace {
  int64_t list, chunk, pnorm, qnorm, col, fpv, fpi, fps, rpv, rps, total;     // byte offsets, each a multiple of 16
};

inline McWorkspace mc_layout(int B, int N, int h, int w) {
  McWorkspace L;
  const int64_t rows = (int64_t)B * N, px = (int64_t)B * h * w, nchunk = (N + MC_CHUNK - 1) / MC_CHUNK;
  L.list = 0;
  L.chunk = L.list + cmr_up16(rows * 4);
  L.pnorm = L.chunk + cmr_up16((int64_t)B * nchunk * 4);
  L.qnorm = L.pnorm + cmr_up16(rows * 4);
  L.col = L.qnorm + cmr_up16(px * 4);
  L.fpv = L.col + cmr_up16(px * 4);
  L.fpi = L.fpv + cmr_up16(MC_SPLITS * rows * 4);
  L.fps = L.fpi + cmr_up16(MC_SPLITS * rows * 4);
  L.rpv = L.fps + cmr_up16(MC_SPLITS * rows * 4);
  L.rps = L.rpv + cmr_up16(MC_SPLITS * px * 4);
  L.total = L.rps + cmr_up16(MC_SPLITS * px * 4);
  return L;
}

}  // namespace

extern "C" int64_t cmr_match_conf_workspace_bytes(int B, int N, int h, int w) {
  return B <= 0 || N <= 0 || h <= 0 || w <= 0 ? 0 : mc_layout(B, N, h, w).total;
}

extern "C" int cmr_match_conf_f32(const float* pc_feat, const float* img_feat, int C, int B, int N, int h, int w, const void* mask,
                                  int mask_bytes, float temperature, float min_conf, const float* gt_xy, float thr, int32_t* idx,
                                  float* conf, uint8_t* keep, int32_t* counts, float* d1, float* row_lse, float* col_lse,
                                  void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  CMR_REQUIRE(pc_feat && img_feat && mask && idx && conf && keep && counts && workspace);
  CMR_REQUIRE(B > 0 && B <= 65535 && N > 0 && h > 0 && w > 0 && (int64_t)h * w <= (int64_t)1 << 24);
  if (C != MC_C) return CMR_EUNSUPPORTED;
  CMR_REQUIRE((int64_t)N <= (int64_t)65535 * MC_CHUNK);
  CMR_REQUIRE(mask_bytes == 1 || mask_bytes == 8);
  CMR_REQUIRE(temperature > 0.f && temperature < __builtin_huge_valf());
  CMR_REQUIRE(min_conf >= 0.f && min_conf <= 1.f);
  CMR_REQUIRE(cmr_aligned16(pc_feat) && cmr_aligned16(img_feat) && cmr_aligned16(workspace));
  CMR_REQUIRE(workspace_bytes >= cmr_match_conf_workspace_bytes(B, N, h, w));
  const McWorkspace L = mc_layout(B, N, h, w);
  char* ws = (char*)workspace;
  int32_t* list = (int32_t*)(ws + L.list);
  int32_t* chunk = (int32_t*)(ws + L.chunk);
  float* pnorm = (float*)(ws + L.pnorm);
  float* qnorm = (float*)(ws + L.qnorm);
  float* col = col_lse ? col_lse : (float*)(ws + L.col);
  float* fpv = (float*)(ws + L.fpv);
  int32_t* fpi = (int32_t*)(ws + L.fpi);
  float* fps = (float*)(ws + L.fps);
  float* rpv = (float*)(ws + L.rpv);
  float* rps = (float*)(ws + L.rps);
  const int hw = h * w, nchunk = (N + MC_CHUNK - 1) / MC_CHUNK;
  const int64_t rows_all = (int64_t)B * N, px_all = (int64_t)B * hw;
  const float kscale = (float)(1.4426950408889634 / (double)temperature);
  const int ft = (hw + MC_TILE - 1) / MC_TILE, rt = (N + MC_TILE - 1) / MC_TILE;
  const int zf = ft < MC_SPLITS ? ft : MC_SPLITS, zr = rt < MC_SPLITS ? rt : MC_SPLITS;      // upper bounds: a range not in use returns
  if (hipMemsetAsync(counts, 0, (size_t)B * 4 * sizeof(int32_t), stream) != hipSuccess) return CMR_ELAUNCH;
  hipLaunchKernelGGL(mc_count_kernel, dim3(nchunk, B), dim3(MC_CHUNK), 0, stream, mask, mask_bytes, N, nchunk, chunk);
  hipLaunchKernelGGL(mc_pack_kernel, dim3(nchunk, B), dim3(MC_CHUNK), 0, stream, mask, mask_bytes, N, nchunk, (const int32_t*)chunk, list,
                     counts);
  const dim3 rows((N + 255) / 256, B), pixels((hw + 255) / 256, B);
  hipLaunchKernelGGL(mc_sweep_kernel<MC_FWD>, dim3(rows.x, B, zf), dim3(MC_THREADS), 0, stream, pc_feat, img_feat, (const int32_t*)list, N, hw,
                     kscale, (const int32_t*)counts, pnorm, fpv, fpi, fps, rows_all);
  hipLaunchKernelGGL(mc_sweep_kernel<MC_REV>, dim3(pixels.x, B, zr), dim3(MC_THREADS), 0, stream, pc_feat, img_feat, (const int32_t*)list, N,
                     hw, kscale, (const int32_t*)counts, qnorm, rpv, (int32_t*)nullptr, rps, px_all);
  hipLaunchKernelGGL(mc_col_kernel, pixels, dim3(256), 0, stream, hw, kscale, temperature, (const int32_t*)counts, (const float*)qnorm,
                     (const float*)rpv, (const float*)rps, px_all, col);
  hipLaunchKernelGGL(mc_final_kernel, rows, dim3(256), 0, stream, mask, mask_bytes, N, hw, w, kscale, temperature, min_conf, gt_xy, thr,
                     (const float*)pnorm, (const float*)fpv, (const int32_t*)fpi, (const float*)fps, rows_all, (const float*)col, idx, conf,
                     keep, d1, row_lse, counts);
  return cmr_launch_status();
}
