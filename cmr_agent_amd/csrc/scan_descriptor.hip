// Place recognition between scans (port extension): Scan Context (Kim & Kim, IROS 2018) restated in include/cmr_hip.h so
// that every integer follows from stated fp32 operations -- no atan2, no fused multiply-add.
//
//   scan_descriptor_kernel   1 024 rows per workgroup, one row per lane and pass: the ring as a count of comparisons against its table, the
//                            sector as cmr_scan_rows.h's azimuth bin (that count, by bisection; both tables in LDS), the value into the
//                            workgroup's image (LDS, <= 16 KiB) by integer atomic max, the image's cells above 0 into desc by integer
//                            atomic max, the three counts by cmr_scan_rows.h's integer atomic adds
//   scan_unit_kernel         the unit columns of a batch of descriptors and their empty flags, one (descriptor, column) per lane
//   scan_match_kernel        a tile of candidates (as many as 256 lanes hold shifts of, at most 16) stays in LDS while the workgroup walks
//                            its queries four at a time: lane (candidate, shift) runs the S columns in order with the four queries'
//                            values from one broadcast 16-byte LDS read and its candidate's from one 4-byte read per ring -- four
//                            products and four sums, unfused by contract, for 6 LDS cycles: the reads, not the arithmetic, bound the
//                            loop; the S distances of a pair go through LDS to the one lane that takes the least in
//                            shift order and stores it
// A maximum and an integer sum are order free and every output of the match is a plain store by its owner: two calls agree bit for bit.
// The ring is a count of at most R - 1 true comparisons, the sector q S / 4 + m with q <= 3 and m the lower end of a search over
// [0, S / 4 - 1], so they lie in [0, R) and [0, S) whatever the rows and the tables hold; a candidate index is below N and a query index
// below Q by the guards at the stores: no store leaves desc, counts, dist and shift.
#include "cmr_scan_rows.h"

#include <math.h>

namespace {

constexpr int MAX_RINGS = 64, MAX_SECTORS = 256, MAX_CELLS = 4096;
constexpr int DESC_ROWS = 1024;                                   // rows per workgroup of the descriptor kernel: four per lane
constexpr int QT = 4;                                             // queries a lane of the match kernel carries at once
constexpr int MAX_TILE = 16;                                      // candidates per workgroup at most

__host__ __device__ inline bool shape_ok(int R, int S) {
  return R >= 1 && R <= MAX_RINGS && S >= 4 && S <= MAX_SECTORS && S % 4 == 0 && R * S <= MAX_CELLS;
}

__global__ __launch_bounds__(256) void scan_descriptor_kernel(const float* __restrict__ pts, int64_t ld, int64_t N, int R, int S,
                                                              const float* __restrict__ ring_edge2, const float* __restrict__ sector_dir,
                                                              float height, int* __restrict__ desc, unsigned long long* __restrict__ counts) {
#pragma clang fp contract(off)
  __shared__ int image[MAX_CELLS];
  __shared__ float edge[MAX_RINGS + 1];
  __shared__ float dirs[MAX_SECTORS / 4][2];
  __shared__ int part[2][4];
  const int cells = R * S, quarter = S / 4;
  for (int c = threadIdx.x; c < cells; c += 256) image[c] = 0;
  for (int j = threadIdx.x; j <= R; j += 256) edge[j] = ring_edge2[j];
  azimuth_load(sector_dir, quarter, dirs);
  __syncthreads();
  int dropped = 0, outside = 0;
  const int64_t first = (int64_t)blockIdx.x * DESC_ROWS;
  for (int p = 0; p < DESC_ROWS / 256; ++p) {
    const int64_t i = first + p * 256 + threadIdx.x;
    if (i >= N) break;
    float x, y, z;
    if (!scan_row(pts, ld, i, x, y, z)) {
      ++dropped;
      continue;
    }
    const float xx = x * x, yy = y * y;
    const float r2 = xx + yy;
    if (r2 < edge[0] || r2 >= edge[R]) {                          // x x may overflow: an infinite r2 is outside
      ++outside;
      continue;
    }
    int ring = 0;
    for (int j = 1; j < R; ++j) ring += r2 >= edge[j] ? 1 : 0;
    const int sector = azimuth_bin(x, y, dirs, quarter);
    const float value = z + height;
    if (value > 0.f) atomicMax(&image[ring * S + sector], __builtin_bit_cast(int, value));      // bits of floats > 0 order like ints
  }
  __syncthreads();
  for (int c = threadIdx.x; c < cells; c += 256) {
    const int v = image[c];
    if (v > 0) atomicMax(&desc[c], v);
  }
  scan_counts_add(dropped, outside, (int)(N - first < DESC_ROWS ? N - first : DESC_ROWS), part, counts);
}

// unit [D][R][S] and full [D][S] (1 = the column is not empty) of descriptors [D][R][S]
__global__ __launch_bounds__(256) void scan_unit_kernel(const float* __restrict__ desc, int64_t D, int R, int S, float* __restrict__ unit,
                                                        float* __restrict__ full) {
#pragma clang fp contract(off)
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= D * S) return;
  const int64_t d = t / S;
  const int j = (int)(t - d * S);
  const float* a = desc + d * R * S + j;
  float n2 = 0.f;
  for (int r = 0; r < R; ++r) {
    const float sq = a[r * S] * a[r * S];
    n2 = n2 + sq;
  }
  const bool empty = n2 == 0.f;
  const float norm = sqrtf(n2);
  float* e = unit + d * R * S + j;
  for (int r = 0; r < R; ++r) e[r * S] = empty ? 0.f : a[r * S] / norm;
  full[t] = empty ? 0.f : 1.f;
}

// LDS of the match kernel, in floats: the candidates' unit columns [tile][R][S] and flags [tile][S], the four queries' unit columns
// [R][S][4] and flags [S][4], the distances of the tile's shifts per query [4][256]
__host__ __device__ inline int match_lds_floats(int R, int S, int tile) { return tile * (R * S + S) + QT * (R * S + S) + QT * 256; }
__host__ inline int match_tile(int S) { return 256 / S < MAX_TILE ? 256 / S : MAX_TILE; }

__global__ __launch_bounds__(256) void scan_match_kernel(const float* __restrict__ qunit, const float* __restrict__ qfull, int Q,
                                                         const float* __restrict__ cunit, const float* __restrict__ cfull, int N, int R, int S,
                                                         int tile, int qgroup, const int32_t* __restrict__ limit, int min_cols,
                                                         float* __restrict__ dist, int32_t* __restrict__ shift) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int cells = R * S;
  float* ec = lds;                                                // [tile][R][S]
  float* fc = ec + tile * cells;                                  // [tile][S]
  f32x4* eq = reinterpret_cast<f32x4*>(fc + tile * S);            // [R][S] of four queries; tile (cells + S) is a multiple of 4: S is
  f32x4* fq = eq + cells;                                         // [S]
  float* dk = reinterpret_cast<float*>(fq + S);                   // [4][256]
  const int c0 = blockIdx.x * tile;
  const int here = N - c0 < tile ? N - c0 : tile;                 // candidates of this tile: >= 1 by the grid
  for (int i = threadIdx.x; i < here * cells; i += 256) ec[i] = cunit[(int64_t)c0 * cells + i];
  for (int i = threadIdx.x; i < here * S; i += 256) fc[i] = cfull[(int64_t)c0 * S + i];
  const int cl = threadIdx.x / S, k = threadIdx.x - cl * S;      // this lane's candidate of the tile and its shift
  const bool lane = cl < here;
  const float* mine = ec + cl * cells;
  const int64_t q_last = ((int64_t)blockIdx.y + 1) * qgroup;
  const int q_end = q_last < Q ? (int)q_last : Q;
  for (int q0 = blockIdx.y * qgroup; q0 < q_end; q0 += QT) {
    const int nq = q_end - q0 < QT ? q_end - q0 : QT;
    int most = 0;                                                 // the largest limit of the four: nothing to compute at or beyond it
    for (int i = 0; i < nq; ++i) {
      const int l = limit ? limit[q0 + i] : N;
      most = l > most ? l : most;
    }
    const bool work = c0 < most;                                  // uniform over the workgroup
    __syncthreads();                                              // the last pass's reads of eq, fq and dk are over; ec and fc are in
    if (work) {
      for (int i = threadIdx.x; i < cells * QT; i += 256) {
        const int qi = i / cells, at = i - qi * cells;
        reinterpret_cast<float*>(eq)[at * QT + qi] = qi < nq ? qunit[(int64_t)(q0 + qi) * cells + at] : 0.f;
      }
      for (int i = threadIdx.x; i < S * QT; i += 256) {
        const int qi = i / S, at = i - qi * S;
        reinterpret_cast<float*>(fq)[at * QT + qi] = qi < nq ? qfull[(int64_t)(q0 + qi) * S + at] : 0.f;
      }
      __syncthreads();
      if (lane) {
        f32x4 sum = {0.f, 0.f, 0.f, 0.f};
        int cnt[QT] = {0, 0, 0, 0};
        int jj = k;                                               // (j + k) mod S
        for (int j = 0; j < S; ++j) {
          f32x4 dot = {0.f, 0.f, 0.f, 0.f};
          for (int r = 0; r < R; ++r) {
            const f32x4 a = eq[r * S + j];
            const float b = mine[r * S + jj];
            const f32x4 prod = a * b;
            dot = dot + prod;
          }
          const f32x4 f = fq[j];
          const bool there = fc[cl * S + jj] != 0.f;
#pragma unroll
          for (int i = 0; i < QT; ++i) {
            const bool both = there && f[i] != 0.f;
            const float next = sum[i] + dot[i];
            sum[i] = both ? next : sum[i];
            cnt[i] += both ? 1 : 0;
          }
          jj = jj + 1 == S ? 0 : jj + 1;
        }
#pragma unroll
        for (int i = 0; i < QT; ++i) {
          const float mean = sum[i] / (float)cnt[i];
          dk[i * 256 + threadIdx.x] = cnt[i] >= min_cols ? 1.f - mean : NAN;      // min_cols >= 1: no division by 0 is kept
        }
      }
      __syncthreads();
    }
    if ((int)threadIdx.x < QT * tile) {                           // one (query, candidate) per lane: the least distance in shift order
      const int qi = threadIdx.x / tile, c = threadIdx.x - qi * tile;
      if (qi < nq && c < here) {
        float best = NAN;
        int at = -1;
        if (work && c0 + c < (limit ? limit[q0 + qi] : N)) {
          for (int s = 0; s < S; ++s) {
            const float d = dk[qi * 256 + c * S + s];
            if (d == d && (at < 0 || d < best)) best = d, at = s;
          }
        }
        dist[(int64_t)(q0 + qi) * N + c0 + c] = best;
        shift[(int64_t)(q0 + qi) * N + c0 + c] = at;
      }
    }
  }
}

CmrSmemCache g_match_smem = {};

}  // namespace

extern "C" int cmr_scan_descriptor_f32(const float* points, int64_t ld, int64_t N, int R, int S, const float* ring_edge2,
                                       const float* sector_dir, float height, float* desc, int64_t* counts, hipStream_t stream) {
  CMR_REQUIRE(points && ld >= 3 && N > 0 && N < ROW_LIMIT && R >= 1 && S >= 1 && ring_edge2 && desc && counts && isfinite(height));
  if (!shape_ok(R, S)) return CMR_EUNSUPPORTED;
  CMR_REQUIRE(S == 4 || sector_dir);
  if (hipMemsetAsync(desc, 0, (size_t)R * S * sizeof(float), stream) != hipSuccess ||
      hipMemsetAsync(counts, 0, 3 * sizeof(int64_t), stream) != hipSuccess)
    return CMR_ELAUNCH;
  const unsigned blocks = (unsigned)((N + DESC_ROWS - 1) / DESC_ROWS);
  hipLaunchKernelGGL(scan_descriptor_kernel, dim3(blocks), dim3(256), 0, stream, points, ld, N, R, S, ring_edge2, sector_dir, height,
                     (int*)desc, (unsigned long long*)counts);
  return cmr_launch_status();
}

extern "C" int64_t cmr_scan_match_workspace_bytes(int64_t Q, int64_t N, int R, int S) {
  return Q > 0 && Q < ROW_LIMIT && N > 0 && N < ROW_LIMIT && shape_ok(R, S) ? (Q + N) * (int64_t)(R * S + S) * 4 : 0;
}

extern "C" int cmr_scan_match_f32(const float* queries, int64_t Q, const float* cands, int64_t N, int R, int S, const int32_t* limit,
                                  int min_cols, float* dist, int32_t* shift, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  CMR_REQUIRE(queries && cands && Q > 0 && Q < ROW_LIMIT && N > 0 && N < ROW_LIMIT && R >= 1 && S >= 1 && dist && shift && workspace &&
              cmr_aligned16(workspace));
  if (!shape_ok(R, S)) return CMR_EUNSUPPORTED;
  CMR_REQUIRE(min_cols >= 1 && min_cols <= S && workspace_bytes >= cmr_scan_match_workspace_bytes(Q, N, R, S));
  const int64_t cells = (int64_t)R * S;
  float* qunit = (float*)workspace;
  float* cunit = qunit + Q * cells;
  float* qfull = cunit + N * cells;
  float* cfull = qfull + Q * S;
  hipLaunchKernelGGL(scan_unit_kernel, dim3((unsigned)((Q * S + 255) / 256)), dim3(256), 0, stream, queries, Q, R, S, qunit, qfull);
  hipLaunchKernelGGL(scan_unit_kernel, dim3((unsigned)((N * S + 255) / 256)), dim3(256), 0, stream, cands, N, R, S, cunit, cfull);
  const int tile = match_tile(S);
  const size_t smem = (size_t)match_lds_floats(R, S, tile) * sizeof(float);
  if (cmr_grant_smem((const void*)scan_match_kernel, smem, g_match_smem) != CMR_OK) return CMR_ELAUNCH;
  // queries per workgroup: enough that a candidate tile's load is a small share of its use, few enough that the grid's y extent fits
  int64_t qgroup = 32;
  while ((Q + qgroup - 1) / qgroup > 65535) qgroup *= 2;
  const dim3 grid((unsigned)((N + tile - 1) / tile), (unsigned)((Q + qgroup - 1) / qgroup));
  hipLaunchKernelGGL(scan_match_kernel, grid, dim3(256), smem, stream, qunit, qfull, (int)Q, cunit, cfull, (int)N, R, S, tile, (int)qgroup,
                     limit, min_cols, dist, shift);
  return cmr_launch_status();
}
