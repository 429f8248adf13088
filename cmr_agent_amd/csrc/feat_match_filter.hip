// Match filtering ahead of PnP-RANSAC (port extension): the nearest pixel feature of every selected point as
// cmr_feat_match_f32 finds it, plus the two classic filters that need a second look at the same 64-channel distance matrix -- the
// mutual check (the pixel's nearest selected point is this point) and Lowe's ratio test against the best pixel OUTSIDE a window around
// the winner -- and an absolute distance bound.
//
// Launches, all enqueued on the caller's stream (the sweeps the flags do not need are skipped):
//   fmf_count_kernel / fmf_pack_kernel  selected rows of every sample -> a row list in ROW ORDER (two-pass count + scan, no atomics: the
//                                       reverse sweep's tie rule is "lowest list position", which must mean "lowest n");
//   fmf_sweep_kernel<FMF_BEST>    queries = listed points, streamed = the sample's pixels: fm_match_kernel's tile shape and arithmetic
//                                 (|q|^2 - 2 p.q on 32x32x2 fp32 MFMA, pixels = A rows from LDS tiles of 64, queries = B columns in
//                                 registers, strict < in increasing pixel order), so idx is cmr_feat_match_f32's idx bit for bit;
//   fmf_best_kernel               folds the splits (below) into idx and d1;
//   fmf_sweep_kernel<FMF_REV>     the same problem with the roles swapped: queries = pixels, streamed = the listed points (gathered
//                                 through the list), result = the row number of the winning list position;  fmf_rev_kernel folds;
//   fmf_sweep_kernel<FMF_SECOND>  the forward sweep again, a candidate counting only when it lies outside the window of the row's best
//                                 pixel (pixel x / y ride in LDS beside the squared norms: one division per staged pixel, none per score);
//   fmf_final_kernel              one thread per row: d2 from its splits, keep, the unselected rows' fill values and the four counts
//                                 (integer atomics).
// Splits: 256 queries per workgroup leave a small problem with fewer workgroups than the 256 CUs hold (40 x 128 pixels are 20 per sample
// in the reverse sweep), so a sweep cuts the STREAMED side into up to FMF_SPLITS contiguous ranges of tiles (gridDim.z), each workgroup
// writes its range's (score, index) to a slot of its own and the fold takes them in range order with the same strict <.  The minimum
// and its lowest index do not depend on where the ranges are cut, so neither does any output (the cut is chosen on the device from the
// sample's own selected count).  Every result is a plain store from the one workgroup / thread that owns it: no floating-point atomics,
// no launch-order dependence.
#include "cmr_common.h"

namespace {

constexpr int FMF_C = 64;         // feature width (the model's only one)
constexpr int FMF_THREADS = 256;  // 4 waves
constexpr int FMF_ROWS = 256;     // queries per workgroup: wave w holds queries 64w .. 64w+63 as two 32-column B tiles
constexpr int FMF_TILE = 64;      // streamed rows per LDS tile: 64 rows of 16 float4 chunks, chunk c of row r stored at c ^ (r & 15)
constexpr int FMF_CHUNK = 256;    // rows per compaction workgroup
constexpr int FMF_SPLITS = 8;     // most ranges the streamed side of a sweep is cut into
constexpr int FMF_TARGET = 1024;  // workgroups a sweep aims for: two full rounds of the 256 CUs x 2 resident workgroups

enum { FMF_BEST = 0, FMF_SECOND = 1, FMF_REV = 2 };

__device__ __forceinline__ unsigned fmf_xhalf_u(unsigned u) {
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return (threadIdx.x & 32) ? r[0] : r[1];
}

// ---- order-preserving compaction ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FMF_CHUNK) void fmf_count_kernel(const void* __restrict__ mask, int mask_bytes, int N, int nchunk,
                                                              int32_t* __restrict__ chunk_cnt) {
  __shared__ int wc[FMF_CHUNK / 64];
  const int b = blockIdx.y, n = blockIdx.x * FMF_CHUNK + threadIdx.x;
  const bool sel = n < N && cmr_sel(mask, mask_bytes, (int64_t)b * N + n);
  const int c = __popcll(__ballot(sel));
  if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) chunk_cnt[(int64_t)b * nchunk + blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

__global__ __launch_bounds__(FMF_CHUNK) void fmf_pack_kernel(const void* __restrict__ mask, int mask_bytes, int N, int nchunk,
                                                             const int32_t* __restrict__ chunk_cnt, int32_t* __restrict__ list,
                                                             int32_t* __restrict__ counts) {
  __shared__ int red[FMF_CHUNK];
  __shared__ int wc[FMF_CHUNK / 64];
  const int b = blockIdx.y, c = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int s = 0;
  for (int i = threadIdx.x; i < c; i += FMF_CHUNK) s += chunk_cnt[(int64_t)b * nchunk + i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int k = FMF_CHUNK / 2; k > 0; k >>= 1) {
    if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  const int base = red[0];
  const int n = c * FMF_CHUNK + threadIdx.x;
  const bool sel = n < N && cmr_sel(mask, mask_bytes, (int64_t)b * N + n);
  const unsigned long long bal = __ballot(sel);
  if (lane == 0) wc[wave] = __popcll(bal);
  __syncthreads();
  int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) pos += wc[w];
  if (sel) list[(int64_t)b * N + pos] = n;
  if (c == nchunk - 1 && threadIdx.x == 0) counts[4 * b] = base + wc[0] + wc[1] + wc[2] + wc[3];   // = the number of selected rows
}

// ---- the distance sweeps -------------------------------------------------------------------------------------------------------------
// Stages streamed rows [j0, j0 + 64) of one sample: thread t loads a quarter row (4 float4) of row t >> 2 into registers.  Forward the
// rows are the pixels themselves, in the reverse sweep the listed points.
template <int MODE>
__device__ __forceinline__ void fmf_load(const float* __restrict__ pc_b, const float* __restrict__ img_b, const int32_t* __restrict__ list_b,
                                         int ns, int j0, float4 (&v)[4]) {
  const int j = j0 + (threadIdx.x >> 2);
  if (j < ns) {
    const float* row = MODE == FMF_REV ? pc_b + (int64_t)list_b[j] * FMF_C : img_b + (int64_t)j * FMF_C;
    const float4* src = reinterpret_cast<const float4*>(row) + 4 * (threadIdx.x & 3);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = src[i];
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// ... and writes them (swizzled) plus the row's squared norm; rows past the end get +inf and are never chosen.  FMF_SECOND also
// leaves the pixel's x and y for the window test.
template <int MODE>
__device__ __forceinline__ void fmf_store(float4* tile, float* qn, int* sx, int* sy, int ns, int w, int j0, const float4 (&v)[4]) {
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
  if (q == 0) {
    qn[r] = j0 + r < ns ? s : __builtin_huge_valf();
    if (MODE == FMF_SECOND) {
      const int y = (j0 + r) / w;
      sy[r] = y;
      sx[r] = j0 + r - y * w;
    }
  }
}

// How a sweep with nq queries and ns streamed rows per sample is cut: -> the number of ranges in use (<= zmax), tps = tiles per range.
// The batch's samples are taken to be alike (nq * B queries in all); sweep and fold call this with the same arguments.
__device__ __forceinline__ int fmf_splits(int nq, int ns, int B, int zmax, int& tps) {
  const int ntile = (ns + FMF_TILE - 1) / FMF_TILE;
  tps = 0;
  if (ntile == 0 || nq == 0) return 0;
  const int64_t qwg = (int64_t)((nq + FMF_ROWS - 1) / FMF_ROWS) * B;
  int want = (int)((FMF_TARGET + qwg - 1) / qwg);
  want = want < zmax ? want : zmax;
  want = want < ntile ? want : ntile;
  want = want > 1 ? want : 1;
  tps = (ntile + want - 1) / want;
  return (ntile + tps - 1) / tps;
}

template <int MODE>
__global__ __launch_bounds__(256) void fmf_sweep_kernel(const float* __restrict__ pc, const float* __restrict__ img, const int32_t* __restrict__ list,
                                                        int N, int hw, int w, int excl, const int32_t* __restrict__ counts,
                                                        const int32_t* __restrict__ idx, float* __restrict__ pnorm,
                                                        float* __restrict__ pv, int32_t* __restrict__ pi, int64_t pstride) {
  __shared__ float4 tile[2][FMF_TILE * 16];
  __shared__ __attribute__((aligned(16))) float qn[2][FMF_TILE];
  __shared__ __attribute__((aligned(16))) int sx[2][MODE == FMF_SECOND ? FMF_TILE : 4];
  __shared__ __attribute__((aligned(16))) int sy[2][MODE == FMF_SECOND ? FMF_TILE : 4];
  const int b = blockIdx.y;
  const int nsel = counts[4 * b];                                   // written by fmf_pack_kernel (an earlier launch on the stream)
  const int nq = MODE == FMF_REV ? hw : nsel;                       // queries (B columns, registers)
  const int ns = MODE == FMF_REV ? nsel : hw;                       // streamed rows (A rows, LDS)
  const int row0 = blockIdx.x * FMF_ROWS;
  if (row0 >= nq) return;
  int tps;
  const int nact = fmf_splits(nq, ns, gridDim.y, gridDim.z, tps);
  if ((int)blockIdx.z >= nact) return;
  const int t_begin = blockIdx.z * tps;
  const int t_end = t_begin + tps < (ns + FMF_TILE - 1) / FMF_TILE ? t_begin + tps : (ns + FMF_TILE - 1) / FMF_TILE;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int half = lane >> 5, col = lane & 31;
  const float* img_b = img + (int64_t)b * hw * FMF_C;
  const float* pc_b = pc + (int64_t)b * N * FMF_C;
  const int32_t* list_b = list + (int64_t)b * N;

  // B operand: lane holds features 32*half .. 32*half+31 of its column's query (k of MFMA step s is 32*half + s, on both operands)
  float bq[2][32];
  int n_of[2];                                                      // forward: the query's row number n; reverse: its pixel
  bool valid[2];
  float pn[2];
  int xlo[2], ylo[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int r = row0 + 64 * wave + 32 * t + col;
    valid[t] = r < nq;
    n_of[t] = valid[t] ? (MODE == FMF_REV ? r : list_b[r]) : 0;
    const float* row = MODE == FMF_REV ? img_b + (int64_t)n_of[t] * FMF_C : pc_b + (int64_t)n_of[t] * FMF_C;
    const float4* src = reinterpret_cast<const float4*>(row + 32 * half);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float4 v = valid[t] ? src[j] : make_float4(0.f, 0.f, 0.f, 0.f);
      bq[t][4 * j] = v.x; bq[t][4 * j + 1] = v.y; bq[t][4 * j + 2] = v.z; bq[t][4 * j + 3] = v.w;
      s = fmaf(v.x, v.x, s); s = fmaf(v.y, v.y, s); s = fmaf(v.z, v.z, s); s = fmaf(v.w, v.w, s);
    }
    pn[t] = s + cmr_xhalf(s);
    xlo[t] = ylo[t] = 0;
    if (MODE == FMF_SECOND) {
      const int p = valid[t] ? idx[(int64_t)b * N + n_of[t]] : 0;   // the best pixel, written by the FMF_BEST sweep
      ylo[t] = p / w - excl;
      xlo[t] = p % w - excl;
    }
  }
  const unsigned span = 2u * (unsigned)excl;                        // inside the window <=> (unsigned)(x - xlo) <= span, y alike

  float best[2] = {__builtin_huge_valf(), __builtin_huge_valf()};
  int bidx[2] = {t_begin * FMF_TILE, t_begin * FMF_TILE};           // all-NaN scores keep the range's first entry, as torch.argmin
  float4 pre[4];
  fmf_load<MODE>(pc_b, img_b, list_b, ns, t_begin * FMF_TILE, pre);
  fmf_store<MODE>(tile[0], qn[0], sx[0], sy[0], ns, w, t_begin * FMF_TILE, pre);
  __syncthreads();
  for (int it = t_begin; it < t_end; ++it) {
    const int buf = (it - t_begin) & 1, p0 = it * FMF_TILE;
    const bool more = it + 1 < t_end;
    if (more) fmf_load<MODE>(pc_b, img_b, list_b, ns, p0 + FMF_TILE, pre);
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
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int o = 32 * u + 8 * g4 + 4 * half;
        const float4 q4 = *reinterpret_cast<const float4*>(&qn[buf][o]);
        const float qv[4] = {q4.x, q4.y, q4.z, q4.w};
        int xv[4] = {0, 0, 0, 0}, yv[4] = {0, 0, 0, 0};
        if (MODE == FMF_SECOND) {
          const int4 x4 = *reinterpret_cast<const int4*>(&sx[buf][o]);
          const int4 y4 = *reinterpret_cast<const int4*>(&sy[buf][o]);
          xv[0] = x4.x; xv[1] = x4.y; xv[2] = x4.z; xv[3] = x4.w;
          yv[0] = y4.x; yv[1] = y4.y; yv[2] = y4.z; yv[3] = y4.w;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int g = 4 * g4 + e;
          const int pix = p0 + o + e;                               // = cmr_mfma_row(g, lane): increasing with g in a lane
          const float v0 = fmaf(-2.f, acc0[g], qv[e]);
          const float v1 = fmaf(-2.f, acc1[g], qv[e]);
          if (MODE == FMF_SECOND) {
            // branch-free (a short-circuit here compiles to a divergent branch per score): the larger of the two unsigned offsets
            // decides, a pixel inside the window scores +inf, and only the minimum is asked
            const unsigned m0 = max((unsigned)(xv[e] - xlo[0]), (unsigned)(yv[e] - ylo[0]));
            const unsigned m1 = max((unsigned)(xv[e] - xlo[1]), (unsigned)(yv[e] - ylo[1]));
            best[0] = fminf(best[0], m0 > span ? v0 : __builtin_huge_valf());
            best[1] = fminf(best[1], m1 > span ? v1 : __builtin_huge_valf());
          } else {
            if (v0 < best[0]) { best[0] = v0; bidx[0] = pix; }      // strict: the first (lowest) entry of a tie stays
            if (v1 < best[1]) { best[1] = v1; bidx[1] = pix; }
          }
        }
      }
    }
    if (more) fmf_store<MODE>(tile[buf ^ 1], qn[buf ^ 1], sx[buf ^ 1], sy[buf ^ 1], ns, w, p0 + FMF_TILE, pre);
    __syncthreads();
  }

  // the two lane halves saw interleaved streamed rows: lower score wins, a tie goes to the lower index
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const float ob = __builtin_bit_cast(float, fmf_xhalf_u(__builtin_bit_cast(unsigned, best[t])));
    const int oi = (int)fmf_xhalf_u((unsigned)bidx[t]);
    if (ob < best[t] || (ob == best[t] && oi < bidx[t])) { best[t] = ob; bidx[t] = oi; }
    if (!(valid[t] && half == 0)) continue;
    const int64_t slot = blockIdx.z * pstride + (MODE == FMF_REV ? (int64_t)b * hw : (int64_t)b * N) + n_of[t];
    pv[slot] = best[t];
    if (MODE == FMF_REV) pi[slot] = list_b[bidx[t]];
    if (MODE == FMF_BEST) {
      pi[slot] = bidx[t];
      if (blockIdx.z == 0) pnorm[(int64_t)b * N + n_of[t]] = pn[t];
    }
  }
}

// ---- folds ---------------------------------------------------------------------------------------------------------------------------
// idx and d1 of every selected row from the FMF_BEST ranges, taken in pixel order: strict <, so the lowest pixel of a tie stays.
__global__ __launch_bounds__(256) void fmf_best_kernel(const void* __restrict__ mask, int mask_bytes, int N, int hw, int zmax,
                                                       const int32_t* __restrict__ counts, const float* __restrict__ pnorm,
                                                       const float* __restrict__ pv, const int32_t* __restrict__ pi, int64_t pstride,
                                                       int32_t* __restrict__ idx, float* __restrict__ d1w) {
  const int b = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
  const int64_t g = (int64_t)b * N + n;
  if (n >= N || !cmr_sel(mask, mask_bytes, g)) return;
  int tps;
  const int nact = fmf_splits(counts[4 * b], hw, gridDim.y, zmax, tps);
  float best = pv[g];
  int p = pi[g];
  for (int z = 1; z < nact; ++z) {
    const float v = pv[z * pstride + g];
    if (v < best) { best = v; p = pi[z * pstride + g]; }
  }
  idx[g] = p;
  d1w[g] = sqrtf(fmaxf(pnorm[g] + best, 0.f));
}

// rev of every pixel from the FMF_REV ranges, taken in list (= row) order; -1 when nothing is selected.
__global__ __launch_bounds__(256) void fmf_rev_kernel(int hw, int zmax, const int32_t* __restrict__ counts, const float* __restrict__ pv,
                                                      const int32_t* __restrict__ pi, int64_t pstride, int32_t* __restrict__ revw) {
  const int b = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
  if (p >= hw) return;
  const int64_t g = (int64_t)b * hw + p;
  int tps;
  const int nact = fmf_splits(hw, counts[4 * b], gridDim.y, zmax, tps);
  int n = -1;
  if (nact > 0) {
    float best = pv[g];
    n = pi[g];
    for (int z = 1; z < nact; ++z) {
      const float v = pv[z * pstride + g];
      if (v < best) { best = v; n = pi[z * pstride + g]; }
    }
  }
  revw[g] = n;
}

// ---- keep + counts -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fmf_final_kernel(const void* __restrict__ mask, int mask_bytes, int N, int hw, int w, int mutual,
                                                        int second, float ratio, float max_dist, const float* __restrict__ gt_xy,
                                                        float thr, int zmax, const float* __restrict__ pnorm, const float* __restrict__ pv,
                                                        int64_t pstride, const float* d1w, const int32_t* __restrict__ revw,
                                                        int32_t* __restrict__ idx, uint8_t* __restrict__ keep, float* d1, float* d2,
                                                        int32_t* __restrict__ counts) {      // d1 may be d1w
  const int b = blockIdx.y;
  const int n = blockIdx.x * 256 + threadIdx.x;
  const int64_t g = (int64_t)b * N + n;
  const int nsel = counts[4 * b];                                   // this kernel adds to the other three entries only
  bool kept = false, inl = false;
  if (n < N) {
    if (cmr_sel(mask, mask_bytes, g)) {
      const int p = idx[g];
      const float a = d1w[g];
      kept = true;
      if (mutual) kept = revw[(int64_t)b * hw + p] == n;
      if (second) {                                                 // the FMF_SECOND ranges: the minimum is all that is asked
        int tps;
        const int nact = fmf_splits(nsel, hw, gridDim.y, zmax, tps);
        float best = pv[g];
        for (int z = 1; z < nact; ++z) best = fminf(best, pv[z * pstride + g]);
        const float c = sqrtf(fmaxf(pnorm[g] + best, 0.f));         // +inf stays +inf: no pixel outside the window
        if (d2) d2[g] = c;
        if (ratio > 0.f) kept = kept && a <= ratio * c;
      }
      if (max_dist > 0.f) kept = kept && a <= max_dist;
      if (gt_xy) {
        const float x = gt_xy[(int64_t)b * 2 * N + n], y = gt_xy[(int64_t)b * 2 * N + N + n];
        const float dx = (float)(p % w) - x, dy = (float)(p / w) - y;
        inl = isfinite(x) && isfinite(y) && sqrtf(dx * dx + dy * dy) <= thr;
      }
    } else {
      idx[g] = -1;
      if (d1) d1[g] = __builtin_nanf("");
      if (d2) d2[g] = __builtin_nanf("");
    }
    keep[g] = kept ? 1 : 0;
  }
  const int c1 = __popcll(__ballot(kept));
  const int c2 = __popcll(__ballot(kept && inl));
  const int c3 = __popcll(__ballot(inl));
  if ((threadIdx.x & 63) == 0) {
    if (c1) atomicAdd(&counts[4 * b + 1], c1);
    if (c2) atomicAdd(&counts[4 * b + 2], c2);
    if (c3) atomicAdd(&counts[4 * b + 3], c3);
  }
}

struct FmfWorkspace {
  int64_t list, chunk, pnorm, d1, rev, pv, pi, pstride, total;      // byte offsets, each a multiple of 16; pstride in elements
};

inline FmfWorkspace fmf_layout(int B, int N, int h, int w) {
  FmfWorkspace L;
  const int64_t rows = (int64_t)B * N, px = (int64_t)B * h * w, nchunk = (N + FMF_CHUNK - 1) / FMF_CHUNK;
  L.pstride = rows > px ? rows : px;                                // a range's slot serves the forward sweeps and the reverse one in turn
  L.list = 0;
  L.chunk = L.list + cmr_up16(rows * 4);
  L.pnorm = L.chunk + cmr_up16((int64_t)B * nchunk * 4);
  L.d1 = L.pnorm + cmr_up16(rows * 4);
  L.rev = L.d1 + cmr_up16(rows * 4);
  L.pv = L.rev + cmr_up16(px * 4);
  L.pi = L.pv + cmr_up16(FMF_SPLITS * L.pstride * 4);
  L.total = L.pi + cmr_up16(FMF_SPLITS * L.pstride * 4);
  return L;
}

// gridDim.z of a sweep with at most nq queries and ns streamed rows per sample: 1 when the queries alone fill the machine even if
// only an eighth of them is selected, never more than there are tiles.
inline int fmf_zmax(int64_t nq, int64_t ns, int B) {
  const int64_t qwg = (nq + FMF_ROWS - 1) / FMF_ROWS * B, ntile = (ns + FMF_TILE - 1) / FMF_TILE;
  int64_t z = qwg / 8 >= FMF_TARGET ? 1 : FMF_SPLITS;
  z = z < ntile ? z : ntile;
  return (int)(z > 1 ? z : 1);
}

}  // namespace

extern "C" int64_t cmr_feat_match_filter_workspace_bytes(int B, int N, int h, int w) {
  return B <= 0 || N <= 0 || h <= 0 || w <= 0 ? 0 : fmf_layout(B, N, h, w).total;
}

extern "C" int cmr_feat_match_filter_f32(const float* pc_feat, const float* img_feat, int C, int B, int N, int h, int w, const void* mask,
                                         int mask_bytes, int mutual, float ratio, int excl_radius, float max_dist, const float* gt_xy,
                                         float thr, int32_t* idx, uint8_t* keep, int32_t* counts, float* d1, float* d2, int32_t* rev,
                                         void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  CMR_REQUIRE(pc_feat && img_feat && mask && idx && keep && counts && workspace);
  CMR_REQUIRE(C == FMF_C && B > 0 && B <= 65535 && N > 0 && h > 0 && w > 0 && (int64_t)h * w <= (int64_t)1 << 30);
  CMR_REQUIRE((int64_t)N <= (int64_t)65535 * FMF_CHUNK);
  CMR_REQUIRE(mask_bytes == 1 || mask_bytes == 8);
  CMR_REQUIRE(excl_radius >= 0 && ratio == ratio && max_dist == max_dist);
  CMR_REQUIRE(cmr_aligned16(pc_feat) && cmr_aligned16(img_feat) && cmr_aligned16(workspace));
  CMR_REQUIRE(workspace_bytes >= cmr_feat_match_filter_workspace_bytes(B, N, h, w));
  const FmfWorkspace L = fmf_layout(B, N, h, w);
  char* ws = (char*)workspace;
  int32_t* list = (int32_t*)(ws + L.list);
  int32_t* chunk = (int32_t*)(ws + L.chunk);
  float* pnorm = (float*)(ws + L.pnorm);
  float* pv = (float*)(ws + L.pv);
  int32_t* pi = (int32_t*)(ws + L.pi);
  float* d1w = d1 ? d1 : (float*)(ws + L.d1);
  int32_t* revw = rev ? rev : (int32_t*)(ws + L.rev);
  const int hw = h * w, nchunk = (N + FMF_CHUNK - 1) / FMF_CHUNK;
  const int excl = excl_radius < (h > w ? h : w) ? excl_radius : (h > w ? h : w);    // a window that covers the map either way; no overflow
  const bool need_rev = mutual != 0 || rev != nullptr;
  const bool need_second = ratio > 0.f || d2 != nullptr;
  const int zf = fmf_zmax(N, hw, B), zr = fmf_zmax(hw, N, B);
  if (hipMemsetAsync(counts, 0, (size_t)B * 4 * sizeof(int32_t), stream) != hipSuccess) return CMR_ELAUNCH;
  hipLaunchKernelGGL(fmf_count_kernel, dim3(nchunk, B), dim3(FMF_CHUNK), 0, stream, mask, mask_bytes, N, nchunk, chunk);
  hipLaunchKernelGGL(fmf_pack_kernel, dim3(nchunk, B), dim3(FMF_CHUNK), 0, stream, mask, mask_bytes, N, nchunk, (const int32_t*)chunk, list,
                     counts);
  const dim3 rows((N + 255) / 256, B), pixels((hw + 255) / 256, B);
  hipLaunchKernelGGL(fmf_sweep_kernel<FMF_BEST>, dim3(rows.x, B, zf), dim3(FMF_THREADS), 0, stream, pc_feat, img_feat, (const int32_t*)list, N,
                     hw, w, excl, (const int32_t*)counts, (const int32_t*)idx, pnorm, pv, pi, L.pstride);
  hipLaunchKernelGGL(fmf_best_kernel, rows, dim3(256), 0, stream, mask, mask_bytes, N, hw, zf, (const int32_t*)counts, (const float*)pnorm,
                     (const float*)pv, (const int32_t*)pi, L.pstride, idx, d1w);
  if (need_rev) {
    hipLaunchKernelGGL(fmf_sweep_kernel<FMF_REV>, dim3(pixels.x, B, zr), dim3(FMF_THREADS), 0, stream, pc_feat, img_feat, (const int32_t*)list,
                       N, hw, w, excl, (const int32_t*)counts, (const int32_t*)idx, pnorm, pv, pi, L.pstride);
    hipLaunchKernelGGL(fmf_rev_kernel, pixels, dim3(256), 0, stream, hw, zr, (const int32_t*)counts, (const float*)pv, (const int32_t*)pi,
                       L.pstride, revw);
  }
  if (need_second)
    hipLaunchKernelGGL(fmf_sweep_kernel<FMF_SECOND>, dim3(rows.x, B, zf), dim3(FMF_THREADS), 0, stream, pc_feat, img_feat, (const int32_t*)list,
                       N, hw, w, excl, (const int32_t*)counts, (const int32_t*)idx, pnorm, pv, pi, L.pstride);
  hipLaunchKernelGGL(fmf_final_kernel, rows, dim3(256), 0, stream, mask, mask_bytes, N, hw, w, mutual != 0 ? 1 : 0, need_second ? 1 : 0, ratio,
                     max_dist, gt_xy, thr, zf, (const float*)pnorm, (const float*)pv, L.pstride, (const float*)d1w, (const int32_t*)revw, idx,
                     keep, d1, d2, counts);
  return cmr_launch_status();
}
