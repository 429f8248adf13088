// Gauss-Newton pose refinement from a GIVEN pose (port extension): the refinement step of cmr_pnp_ransac_f32 (DESIGN.md
// 4l, csrc/pnp.hip pnp_select_kernel) from any start pose, with the accumulation split over the correspondences instead of running in
// one workgroup per sample.  The two share their pieces through cmr_pnp.h: the inlier test, one correspondence's terms (cmr_pnp_terms),
// the Cholesky solve, the working pose's load, left update and fp32 4x4 form, and the slice-order sum.
//
// Launches, all on the caller's stream; the sequence depends on `iters` alone (3 + 2 (iters + 1) launches), a sample that has stopped
// turns its remaining launches into early returns read from its state in the workspace:
//   prf_init_kernel    per sample: pose_in -> the float64 working pose, K[R|t] of pose_in rounded to fp32 (the working set's predicate);
//   for it = 0 .. iters:
//     prf_accum_kernel   grid (slices, B), a slice = PRF_SLICE consecutive rows: the rows of the slice that are selected AND inliers of
//                        pose_in (cmr_pnp.h: RANSAC's own inlier test) add their J^T J (21), J^T r (6) and cost (1) in float64 -- per
//                        thread in row order (rows t, t + 256, ...), wave butterfly, the four waves in order -- into the slice's own
//                        slot, with the integer size of the slice's share of the working set.  Rows need no compaction;
//     prf_step_kernel    per sample: adds the slots IN SLICE ORDER, then the accept / undo logic of pnp_select_kernel: a cost that did
//                        not drop undoes the last step and stops; otherwise 6x6 Cholesky, left increment X_c <- Exp(w) X_c + v;
//   prf_count_kernel   grid (slices, B): inliers of the working pose over ALL selected rows, per slice (integers);
//   prf_final_kernel   per sample: adds the slice counts, keeps the refined pose if the count is >= the working set's size.
// No floating-point atomics, no atomics at all: every slot, state and output has one writer, and the slice size is a constant, so two
// calls agree bit for bit and a sample depends on its own rows only.
#include "cmr_pnp.h"

namespace {

constexpr int PRF_THREADS = 256;
constexpr int PRF_SLICE = 1024;      // rows per accumulation workgroup: 4 per thread.  A constant: the summation order must not depend on B
constexpr int PRF_NACC = CMR_GN_NACC; // J^T J (21 upper-triangle entries), J^T r (6), cost

struct PrfState {
  double cur[12];                    // the working pose: R row-major, t
  double prev[12];
  double cost_prev;
  float Min[12];                     // K [R|t] of pose_in in fp32: the working set's predicate
  int32_t stop, status, wcount, pad;
};

__global__ __launch_bounds__(64) void prf_init_kernel(const float* __restrict__ pose_in, const float* __restrict__ Kin,
                                                      PrfState* __restrict__ state) {
  const int b = blockIdx.x;
  if (threadIdx.x != 0) return;
  PrfState& st = state[b];
  const float* P = pose_in + 16 * b;
  double K[9];
  for (int i = 0; i < 9; ++i) K[i] = (double)Kin[9 * b + i];
  cmr_pose_load(P, st.cur);
  for (int i = 0; i < 12; ++i) st.prev[i] = st.cur[i];
  st.cost_prev = 0.0;
  cmr_pnp_kmat(K, st.cur, st.cur + 9, st.Min);
  st.stop = 0;
  st.status = 0;
  st.wcount = 0;
  st.pad = 0;
}

__global__ __launch_bounds__(PRF_THREADS) void prf_accum_kernel(const float* __restrict__ pts, const float* __restrict__ uv,
                                                                const void* __restrict__ mask, int mask_bytes,
                                                                const float* __restrict__ Kin, int N, float thr2,
                                                                const PrfState* __restrict__ state, double* __restrict__ slots,
                                                                int32_t* __restrict__ cslots) {
  __shared__ double acc[PRF_THREADS / 64][PRF_NACC];
  __shared__ int cnt[PRF_THREADS / 64];
  const int b = blockIdx.y, s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const PrfState& st = state[b];
  if (st.stop) return;
  double R[9], t[3], K[9];
  float Min[12];
  for (int i = 0; i < 9; ++i) R[i] = st.cur[i];
  for (int i = 0; i < 3; ++i) t[i] = st.cur[9 + i];
  for (int i = 0; i < 12; ++i) Min[i] = st.Min[i];
  for (int i = 0; i < 9; ++i) K[i] = (double)Kin[9 * b + i];
  const float* pb = pts + (int64_t)b * 3 * N;
  const float* qb = uv + (int64_t)b * 2 * N;
  const int end = (s + 1) * PRF_SLICE < N ? (s + 1) * PRF_SLICE : N;
  double a[PRF_NACC] = {};
  int c = 0;
  for (int i = s * PRF_SLICE + tid; i < end; i += PRF_THREADS) {
    if (!cmr_sel(mask, mask_bytes, (int64_t)b * N + i)) continue;
    const float X = pb[i], Y = pb[N + i], Z = pb[2 * N + i], u = qb[i], v = qb[N + i];
    if (!cmr_pnp_inlier(Min, X, Y, Z, u, v, thr2)) continue;
    ++c;
    cmr_pnp_terms(K, R, t, X, Y, Z, u, v, a);
  }
#pragma unroll
  for (int q = 0; q < PRF_NACC; ++q) {
    const double v = cmr_wave_sum_d(a[q]);
    if (lane == 0) acc[wave][q] = v;
  }
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if (lane == 0) cnt[wave] = c;
  __syncthreads();
  const int64_t slot = (int64_t)b * gridDim.x + s;
  if (tid < PRF_NACC) {
    double v = acc[0][tid];
    for (int w = 1; w < PRF_THREADS / 64; ++w) v += acc[w][tid];
    slots[slot * PRF_NACC + tid] = v;
  }
  if (tid == 64) cslots[slot] = cnt[0] + cnt[1] + cnt[2] + cnt[3];
}

__global__ __launch_bounds__(64) void prf_step_kernel(int it, int iters, int nslice, PrfState* __restrict__ state,
                                                      const double* __restrict__ slots, const int32_t* __restrict__ cslots) {
  __shared__ double tot[PRF_NACC];
  __shared__ int wc;
  const int b = blockIdx.x, tid = threadIdx.x;
  PrfState& st = state[b];
  if (st.stop) return;
  if (tid < PRF_NACC) {
    tot[tid] = cmr_slot_sum(slots + (int64_t)b * nslice * PRF_NACC, nslice, tid);
  } else if (tid == PRF_NACC) {
    int c = 0;
    for (int s = 0; s < nslice; ++s) c += cslots[(int64_t)b * nslice + s];
    wc = c;
  }
  __syncthreads();
  if (tid != 0) return;
  if (it == 0) {
    st.wcount = wc;
    if (wc < 4) { st.status = 1; st.stop = 1; return; }
    bool fin = true;
    for (int q = 0; q < PRF_NACC; ++q) fin = fin && isfinite(tot[q]);
    if (!fin) { st.status = 2; st.stop = 1; return; }
  }
  const double cost = tot[27];
  if (it > 0 && !(cost < st.cost_prev)) {
    for (int i = 0; i < 12; ++i) st.cur[i] = st.prev[i];                // the step did not lower the cost: undo it
    st.stop = 1;
    return;
  }
  if (it == iters) { st.stop = 1; return; }
  double g[6], dx[6];
  for (int r = 0; r < 6; ++r) g[r] = -tot[21 + r];
  double nw[12];
  if (!(cmr_pnp_chol6<true>(tot, g, dx) && cmr_pose_left_update(st.cur, dx, nw))) {
    if (it == 0) st.status = 2;                                          // nothing to refine with: the call returns pose_in
    st.stop = 1;
    return;
  }
  for (int i = 0; i < 12; ++i) { st.prev[i] = st.cur[i]; st.cur[i] = nw[i]; }
  st.cost_prev = cost;
}

__global__ __launch_bounds__(PRF_THREADS) void prf_count_kernel(const float* __restrict__ pts, const float* __restrict__ uv,
                                                                const void* __restrict__ mask, int mask_bytes,
                                                                const float* __restrict__ Kin, int N, float thr2,
                                                                const PrfState* __restrict__ state, int32_t* __restrict__ cslots) {
  __shared__ int cnt[PRF_THREADS / 64];
  const int b = blockIdx.y, s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const PrfState& st = state[b];
  if (st.status != 0) return;
  double K[9];
  for (int i = 0; i < 9; ++i) K[i] = (double)Kin[9 * b + i];
  float M[12];
  cmr_pnp_kmat(K, st.cur, st.cur + 9, M);
  const float* pb = pts + (int64_t)b * 3 * N;
  const float* qb = uv + (int64_t)b * 2 * N;
  const int end = (s + 1) * PRF_SLICE < N ? (s + 1) * PRF_SLICE : N;
  int c = 0;
  for (int i = s * PRF_SLICE + tid; i < end; i += PRF_THREADS)
    if (cmr_sel(mask, mask_bytes, (int64_t)b * N + i)) c += cmr_pnp_inlier(M, pb[i], pb[N + i], pb[2 * N + i], qb[i], qb[N + i], thr2);
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if (lane == 0) cnt[wave] = c;
  __syncthreads();
  if (tid == 0) cslots[(int64_t)b * gridDim.x + s] = cnt[0] + cnt[1] + cnt[2] + cnt[3];
}

__global__ __launch_bounds__(64) void prf_final_kernel(const float* __restrict__ pose_in, int nslice, const PrfState* __restrict__ state,
                                                       const int32_t* __restrict__ cslots, float* __restrict__ pose,
                                                       int32_t* __restrict__ inliers, int32_t* __restrict__ status) {
  __shared__ int sh_use, sh_rc;
  const int b = blockIdx.x, tid = threadIdx.x;
  const PrfState& st = state[b];
  if (tid == 0) {
    int rc = 0, use = 0;
    if (st.status == 0) {
      for (int s = 0; s < nslice; ++s) rc += cslots[(int64_t)b * nslice + s];
      bool fin = true;
      for (int i = 0; i < 12; ++i) fin = fin && isfinite(st.cur[i]);
      use = fin && rc >= st.wcount;
    }
    sh_use = use;
    sh_rc = rc;
    inliers[b] = use ? rc : st.wcount;
    status[b] = st.status != 0 ? st.status : (use ? 0 : 2);
  }
  __syncthreads();
  if (tid < 16) pose[16 * b + tid] = sh_use ? cmr_pose_entry(st.cur, tid) : pose_in[16 * b + tid];
}

struct PrfWs { int64_t state, slots, cslots, total; };

inline PrfWs prf_layout(int B, int N) {
  PrfWs L;
  const int64_t nslice = ((int64_t)N + PRF_SLICE - 1) / PRF_SLICE;
  L.state = 0;
  L.slots = L.state + cmr_up16((int64_t)B * sizeof(PrfState));
  L.cslots = L.slots + cmr_up16((int64_t)B * nslice * PRF_NACC * 8);
  L.total = L.cslots + cmr_up16((int64_t)B * nslice * 4);
  return L;
}

}  // namespace

extern "C" int64_t cmr_pnp_refine_workspace_bytes(int B, int N) { return B <= 0 || N <= 0 ? 0 : prf_layout(B, N).total; }

extern "C" int cmr_pnp_refine_f32(const float* pts, const float* uv, const void* mask, int mask_bytes, const float* K, const float* pose_in,
                                  int B, int N, float thr, int iters, float* pose, int32_t* inliers, int32_t* status, void* ws,
                                  int64_t ws_bytes, hipStream_t stream) {
  CMR_REQUIRE(pts && uv && mask && K && pose_in && pose && inliers && status && ws);
  CMR_REQUIRE(B > 0 && B <= 65535 && N > 0 && (int64_t)N <= (int64_t)65535 * PRF_SLICE && iters >= 0 && iters <= 1000);
  CMR_REQUIRE(mask_bytes == 1 || mask_bytes == 8);
  CMR_REQUIRE(thr > 0.f && __builtin_isfinite(thr));
  CMR_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15u) == 0);
  CMR_REQUIRE(ws_bytes >= cmr_pnp_refine_workspace_bytes(B, N));
  const PrfWs L = prf_layout(B, N);
  PrfState* state = (PrfState*)((char*)ws + L.state);
  double* slots = (double*)((char*)ws + L.slots);
  int32_t* cslots = (int32_t*)((char*)ws + L.cslots);
  const int nslice = (N + PRF_SLICE - 1) / PRF_SLICE;
  const float thr2 = thr * thr;
  hipLaunchKernelGGL(prf_init_kernel, dim3(B), dim3(64), 0, stream, pose_in, K, state);
  for (int it = 0; it <= iters; ++it) {
    hipLaunchKernelGGL(prf_accum_kernel, dim3(nslice, B), dim3(PRF_THREADS), 0, stream, pts, uv, mask, mask_bytes, K, N, thr2,
                       (const PrfState*)state, slots, cslots);
    hipLaunchKernelGGL(prf_step_kernel, dim3(B), dim3(64), 0, stream, it, iters, nslice, state, (const double*)slots, (const int32_t*)cslots);
  }
  hipLaunchKernelGGL(prf_count_kernel, dim3(nslice, B), dim3(PRF_THREADS), 0, stream, pts, uv, mask, mask_bytes, K, N, thr2,
                     (const PrfState*)state, cslots);
  hipLaunchKernelGGL(prf_final_kernel, dim3(B), dim3(64), 0, stream, pose_in, nslice, (const PrfState*)state, (const int32_t*)cslots, pose,
                     inliers, status);
  return cmr_launch_status();
}
