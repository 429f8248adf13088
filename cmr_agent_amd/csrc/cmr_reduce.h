// The second stage of the training kernels' two-stage reductions, stated once.  A first-stage kernel leaves fp32 partials
// per workgroup; the pieces here add them in double in a FIXED order, so a result never depends on scheduling and the data-parallel ranks
// of utils/flatbucket.py stay bit-identical after the all-reduce.  Every caller's bits depend on these orders: change one here and it
// changes for all of them at once, which is the point.
#pragma once
#include "cmr_common.h"

// ---- strided slices: thread (output o, slice group g) of a [GRP][outputs] workgroup ------------------------------------------------
// p[0], p[stride], ... are one output's nslices partials.  Group g adds slices g, g + GRP, g + 2 GRP, ... in ascending order with U
// independent loads in flight (one dependent load per iteration leaves the sum a chain of memory round trips: 28 us for a transformer
// block's gradients, 30-35 us for a 768-slice linear gradient).  Branch-free: a slice past the end re-reads j0 and is dropped, which
// keeps the order of a tail loop.
template <int GRP, int U>
__device__ __forceinline__ double cmr_slice_sum(const float* __restrict__ p, int64_t stride, int nslices, int g) {
  double s = 0.0;
  for (int j0 = g; j0 < nslices; j0 += GRP * U) {
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u * GRP;
      v[u] = p[(int64_t)(j < nslices ? j : j0) * stride];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) s += j0 + u * GRP < nslices ? (double)v[u] : 0.0;
  }
  return s;
}

// The GRP group sums of output o through LDS: group 0 returns ((s_0 + s_1) + s_2) + ... in ascending order where the output exists
// (`live`; the other threads their own sum).  Called by every thread of the workgroup.
template <int GRP, int OUT>
__device__ __forceinline__ double cmr_group_sum(double (&sm)[GRP][OUT], double s, int g, int o, bool live) {
  sm[g][o] = s;
  __syncthreads();
  if (g == 0 && live) {
#pragma unroll
    for (int j = 1; j < GRP; ++j) s += sm[j][o];
  }
  return s;
}

// ---- one wave per output: lane l adds partials l, l + 64, ... in double (U loads per column in flight, added in ascending order), then
// the butterfly of cmr_wave_sum_d.  N columns p, p + col, ... share the pass (a BatchNorm's two sums); every lane returns the totals.
// The count keeps its caller's type (int, or int64_t where a producer leaves the parts): the loop counter follows it.
template <int U, int N, typename I>
__device__ __forceinline__ void cmr_wave_partials_sum(const float* __restrict__ p, int64_t stride, int64_t col, I n, int lane, double (&s)[N]) {
#pragma unroll
  for (int c = 0; c < N; ++c) s[c] = 0.0;
  for (I b0 = lane; b0 < n; b0 += 64 * U) {
    float v[U][N];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t b = b0 + 64 * u < n ? b0 + 64 * u : b0;
#pragma unroll
      for (int c = 0; c < N; ++c) v[u][c] = p[b * stride + c * col];
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (b0 + 64 * u < n) {
#pragma unroll
        for (int c = 0; c < N; ++c) s[c] += (double)v[u][c];
      }
  }
#pragma unroll
  for (int c = 0; c < N; ++c) s[c] = cmr_wave_sum_d(s[c]);
}
template <int U, typename I>
__device__ __forceinline__ double cmr_wave_partials_sum(const float* __restrict__ p, int64_t stride, I n, int lane) {
  double s[1];
  cmr_wave_partials_sum<U, 1>(p, stride, 0, n, lane, s);
  return s[0];
}

// ---- BatchNorm, training mode: from channel c's (mean, biased variance) in double to stat = (mean, rstd, scale, shift) [4][C] and the
// running statistics (unbiased variance), as every statistics kernel leaves them
__device__ __forceinline__ void cmr_bn_stat_tail(double mean, double var, int64_t rows, int c, int C, float eps, float momentum,
                                                 const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ running_mean,
                                                 float* __restrict__ running_var, float* __restrict__ stat) {
  const double n = (double)rows;
  var = var > 0.0 ? var : 0.0;
  const float rstd = (float)(1.0 / sqrt(var + (double)eps));
  const float g = gamma ? gamma[c] : 1.f, bt = beta ? beta[c] : 0.f;
  const float scale = g * rstd;
  stat[c] = (float)mean;
  stat[C + c] = rstd;
  stat[2 * C + c] = scale;
  stat[3 * C + c] = bt - (float)mean * scale;
  if (running_mean) {
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * (float)mean;
    const double unbiased = rows > 1 ? var * n / (n - 1.0) : var;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unbiased;
  }
}

// Parallel variance over workgroups w with pivot p_w, row count n_w, s_w = sum (x - p_w), ss_w = sum (x - p_w)^2, from ONE pass over the
// partials: with d_w = mean - p_w,  M2 = sum_w [ss_w - 2 d_w s_w + n_w d_w^2]
//   = sum ss - 2 mean sum s + 2 sum p s + mean^2 sum n - 2 mean sum n p + sum n p^2   (double: the terms are <= rows * mean^2 ~ 1e8, M2 ~ 1e6)
// The five sums in: s_s = sum s, s_ss = sum ss, s_ps = sum p s, s_np = sum n p, s_npp = sum n p^2.  Returns the biased variance.
__device__ __forceinline__ double cmr_bn_merge5(double s_s, double s_ss, double s_ps, double s_np, double s_npp, int64_t rows, double& mean) {
  const double n = (double)rows;
  mean = (s_np + s_s) / n;
  const double m2 = s_ss - 2.0 * mean * s_s + 2.0 * s_ps + mean * mean * n - 2.0 * mean * s_np + s_npp;
  return m2 / n;
}

// ---- the two second-stage kernels that two sources launch.  Internal linkage, and templates on their loads in flight so that only an
// object file that launches one holds a copy (a plain static kernel is emitted into every file that includes this header). -------------
// coef[0][c] = sum dy / n, coef[1][c] = sum dy xhat / n over part [nblk][2][C];  dgamma / dbeta written into the gradient bucket when given
template <int U>
static __global__ __launch_bounds__(64) void bn_bwd_final_kernel(const float* __restrict__ part, int nblk, int64_t rows, int C, float* __restrict__ coef,
                                                                 float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int c = blockIdx.x, lane = threadIdx.x;
  double s[2];                                     // (sum dy, sum dy xhat)
  cmr_wave_partials_sum<U, 2>(part + c, 2 * C, C, nblk, lane, s);
  if (lane != 0) return;
  coef[c] = (float)(s[0] / (double)rows);
  coef[C + c] = (float)(s[1] / (double)rows);
  if (dbeta) dbeta[c] = (float)s[0];
  if (dgamma) dgamma[c] = (float)s[1];
}

// Linear weight gradient: the slices of one (n block, k block) of part [kblk][nblk][nslices][npad][kpad] (and of part_b [nblk][nslices][npad]).
// Whole-gradient partials [nslices][n][k] are the case nblk = 1, npad = n, kpad = k.
// outputs [0, n k): dW entries; [n k, n k + n): db entries (when part_b)
// (round 3) A thread used to walk its 96 slices of a 768-slice sum one dependent load at a time: 130 workgroups of 256 threads took 30-35 us
// for 12.8 MB (profiles/r03_pmc_lwgrad.txt: 92 % of the wave cycles waiting on memory) -- more than a third of the weight gradient of a
// 524 288-row map.  Now 32 slice groups (1 024 threads) and LRED_U independent loads in flight per thread; sums still in double, fixed order.
constexpr int RED_OUT = 32, LRED_GRP = 32, LRED_U = 8;
template <int U>
static __global__ __launch_bounds__(RED_OUT * LRED_GRP) void linear_wgrad_reduce_kernel(const float* __restrict__ part, const float* __restrict__ part_b,
                                                                                       int nslices, int npad, int kpad, int nblk, int n, int k,
                                                                                       float* __restrict__ dw, int64_t lddw, int accumulate,
                                                                                       float* __restrict__ db, int acc_db) {
  __shared__ double sm[LRED_GRP][RED_OUT];
  const int o = threadIdx.x % RED_OUT, g = threadIdx.x / RED_OUT;
  const int64_t i = (int64_t)blockIdx.x * RED_OUT + o;
  const int64_t nk = (int64_t)n * k, total = nk + (part_b ? n : 0);
  int row = 0, col = 0;
  const float* p = part;
  int64_t stride = 0;
  if (i < nk) {
    row = (int)(i / k), col = (int)(i - (int64_t)row * k);
    const int nb = row / npad, kb = col / kpad;
    p = part + ((int64_t)kb * nblk + nb) * nslices * npad * kpad + (int64_t)(row - nb * npad) * kpad + (col - kb * kpad);
    stride = (int64_t)npad * kpad;
  } else if (i < total) {
    row = (int)(i - nk);
    const int nb = row / npad;
    p = part_b + (int64_t)nb * nslices * npad + (row - nb * npad);
    stride = npad;
  }
  const double s = cmr_group_sum(sm, i < total ? cmr_slice_sum<LRED_GRP, U>(p, stride, nslices, g) : 0.0, g, o, i < total);
  if (g == 0 && i < total) {
    if (i < nk) {
      float* d = dw + (int64_t)row * lddw + col;
      *d = accumulate ? *d + (float)s : (float)s;
    } else {
      db[row] = acc_db ? db[row] + (float)s : (float)s;
    }
  }
}
// launch of linear_wgrad_reduce_kernel over n k (+ n when part_b) outputs (a template for the same reason as the kernel)
template <int U = LRED_U>
static inline void cmr_linear_wgrad_reduce(const float* part, const float* part_b, int nslices, int npad, int kpad, int nblk, int n, int k, float* dw,
                                           int64_t lddw, int accumulate, float* db, int acc_db, hipStream_t stream) {
  const int64_t outs = (int64_t)n * k + (part_b ? n : 0);
  hipLaunchKernelGGL(linear_wgrad_reduce_kernel<U>, dim3((unsigned)((outs + RED_OUT - 1) / RED_OUT)), dim3(RED_OUT * LRED_GRP), 0, stream, part, part_b,
                     nslices, npad, kpad, nblk, n, k, dw, lddw, accumulate, db, acc_db);
}
