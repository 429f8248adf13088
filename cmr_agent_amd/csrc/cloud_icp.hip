// Cloud against cloud on the sorted-key grid (port extension): the nearest target row of every query row, and point-to-plane
// ICP -- the whole Gauss-Newton loop on the device -- on top of it.  The target is a grid index as ops.point_normals builds it
// (cmr_cloud_grid.h: keys, cells, runs; cmr_cloud_gather4_f32: the rows in key order), built once and searched by every call.
//
//   cmr_cloud_nearest_f32        one 16-lane group per query: the runs of the cells round the query (9, more on a cell face), every lane
//                                keeps its least (d2, row), a 16-lane minimum decides.  (d2, row) is ordered lexicographically, so the result
//                                does not depend on which lane met which row: exact, and the same bits in every call.
//   cmr_icp_point_to_plane_f32   launches, all on the caller's stream, 2 iters + 2 whatever the data:
//     icp_init_kernel    pose_in -> the float64 working pose; trace and system = 0;
//     for k = 0 .. iters - 1:
//       icp_accum_kernel   a workgroup = ICP_SLICE consecutive source rows, 16 groups of 16 lanes, a group takes rows g, g + 16, ... of the
//                          slice one after the other: match under the working pose rounded to fp32, then lane 0 of the group adds the
//                          pair's w J^T J (21), w J r (6) and w r^2 in float64.  The 16 group sums are added in group order into the
//                          slice's own slot, the pair counts next to them;
//       icp_step_kernel    one workgroup: adds the slots IN SLICE ORDER, 6x6 Cholesky, T <- [exp(w) | v] T (all three of cmr_pnp.h), trace,
//                          the stop flag;
//     icp_final_kernel   the working pose as fp32, status.
// A call that has stopped turns its remaining launches into early returns read from its state in the workspace.  No atomics: every slot,
// state and output has one writer.  The index (GridIndex), the cells round a query (Walk) and the walk over their runs (walk16) are
// cmr_cloud_grid.h's; the working pose's load, left update and fp32 4x4 form and the slice-order sum are cmr_pnp.h's.
#include "cmr_cloud_grid.h"
#include "cmr_pnp.h"

namespace {

constexpr int ICP_SLICE = 32;        // source rows per accumulation workgroup: 2 per group.  A constant: the summation order rests on it
constexpr int ICP_NACC = CMR_GN_NACC; // H upper triangle (21), g (6), cost
constexpr int NO_ROW = INT32_MAX;

struct IcpState {
  double cur[12];                    // the working pose: R row-major, t
  int32_t stop, code, executed, pad;
};

// The nearest target row of q for one 16-lane group (every lane of the wave calls it; `live` is uniform over the group, as walk16 asks):
// the least d2 among the rows with d2 <= r2, on equal d2 the lowest original row.  -> row (NO_ROW: none), d2, and pos = its place in key order.
__device__ __forceinline__ void nearest16(float qx, float qy, float qz, bool live, const GridIndex& index, float r2, int lane, int& row,
                                          float& best, int& pos) {
  const Walk w(qx, qy, qz, live, index);
  row = NO_ROW;
  best = INFINITY;
  pos = 0;
  walk16(index, w, lane, [&](int64_t j, const f32x4& c) {
    const float dx = c.x - qx, dy = c.y - qy, dz = c.z - qz;
    const float d2 = dist2(dx, dy, dz);
    if (within(dx, dy, dz, r2) && d2 <= best) {
      const int cand = (int)index.order[j];
      if (d2 < best || cand < row) {
        best = d2;
        row = cand;
        pos = (int)j;
      }
    }
  });
  // every lane of the wave is here again: the 16-lane minimum of (d2, row)
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) {
    const float od = __shfl_xor(best, o, 16);
    const int orow = __shfl_xor(row, o, 16), opos = __shfl_xor(pos, o, 16);
    if (od < best || (od == best && orow < row)) {
      best = od;
      row = orow;
      pos = opos;
    }
  }
}

__global__ __launch_bounds__(256) void cloud_nearest_kernel(const float* __restrict__ queries, int64_t ld, int64_t M,
                                                            const float* __restrict__ pose, GridIndex index, float r2,
                                                            int32_t* __restrict__ idx, float* __restrict__ d2out) {
  const int lane = threadIdx.x & 15;
  const int64_t i = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const bool have = i < M;
  const float* p = queries + (have ? i : 0) * ld;
  float qx = p[0], qy = p[1], qz = p[2];
  if (pose) {
    float T[12];
    pose_load(pose, T);
    pose_apply(T, qx, qy, qz, qx, qy, qz);
  }
  int row, pos;
  float best;
  nearest16(qx, qy, qz, have && cmr_finite3(qx, qy, qz), index, r2, lane, row, best, pos);
  if (lane != 0 || !have) return;
  idx[i] = row == NO_ROW ? -1 : row;
  d2out[i] = row == NO_ROW ? NAN : best;
}

// ------------------------------------------------------------------------------------------------------------------------------ ICP
__global__ __launch_bounds__(256) void icp_init_kernel(const float* __restrict__ pose_in, int iters, IcpState* __restrict__ st,
                                                       double* __restrict__ trace, double* __restrict__ system) {
  for (int i = threadIdx.x; i < iters * 4; i += 256) trace[i] = 0.0;
  if (system)
    for (int i = threadIdx.x; i < iters * ICP_NACC; i += 256) system[i] = 0.0;
  if (threadIdx.x != 0) return;
  cmr_pose_load(pose_in, st->cur);
  st->stop = 0;
  st->code = 1;                      // iterations exhausted, until a step says otherwise
  st->executed = 0;
  st->pad = 0;
}

// one pair's terms, in fp64 from the fp32 q, c and n; every operation rounded on its own so that a float64 restatement has the same terms
__device__ __forceinline__ void icp_pair(float qx, float qy, float qz, const f32x4& c, float nx, float ny, float nz, double huber,
                                         double (&a)[ICP_NACC]) {
#pragma clang fp contract(off)
  const double Qx = qx, Qy = qy, Qz = qz, Nx = nx, Ny = ny, Nz = nz;
  const double r = (Nx * (Qx - (double)c.x) + Ny * (Qy - (double)c.y)) + Nz * (Qz - (double)c.z);
  const double J[6] = {Qy * Nz - Qz * Ny, Qz * Nx - Qx * Nz, Qx * Ny - Qy * Nx, Nx, Ny, Nz};
  const double w = huber > 0.0 && fabs(r) > huber ? huber / fabs(r) : 1.0;
  int q = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double wj = w * J[i];
#pragma unroll
    for (int j = i; j < 6; ++j) a[q++] += wj * J[j];
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) a[21 + i] += (w * J[i]) * r;
  a[27] += (w * r) * r;
}

__global__ __launch_bounds__(256) void icp_accum_kernel(const float* __restrict__ src, int64_t ld, int64_t M, GridIndex index,
                                                        const float* __restrict__ normals, float r2, float huber,
                                                        const IcpState* __restrict__ st, double* __restrict__ slots,
                                                        int32_t* __restrict__ cslots) {
  __shared__ double acc[16][ICP_NACC];
  __shared__ int cnt[16];
  if (st->stop) return;
  const int tid = threadIdx.x, lane = tid & 15, g = tid >> 4;
  float T[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) T[i] = (float)st->cur[i];          // the working pose rounded to fp32: what the match sees
  double a[ICP_NACC] = {};
  int pairs = 0;
  const int64_t first = (int64_t)blockIdx.x * ICP_SLICE;
  for (int k = 0; k < ICP_SLICE / 16; ++k) {
    const int64_t i = first + 16 * k + g;
    const bool have = i < M;
    const float* p = src + (have ? i : 0) * ld;
    float qx, qy, qz;
    pose_apply(T, p[0], p[1], p[2], qx, qy, qz);
    int row, pos;
    float best;
    nearest16(qx, qy, qz, have && cmr_finite3(qx, qy, qz), index, r2, lane, row, best, pos);
    if (lane == 0 && row != NO_ROW) {
      const float nx = normals[(int64_t)row * 3], ny = normals[(int64_t)row * 3 + 1], nz = normals[(int64_t)row * 3 + 2];
      if (nx != 0.f || ny != 0.f || nz != 0.f) {
        icp_pair(qx, qy, qz, index.pts4[pos], nx, ny, nz, (double)huber, a);
        ++pairs;
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < ICP_NACC; ++q) acc[g][q] = a[q];
    cnt[g] = pairs;
  }
  __syncthreads();
  if (tid < ICP_NACC) {
    double v = acc[0][tid];
    for (int w = 1; w < 16; ++w) v += acc[w][tid];                  // group order
    slots[(int64_t)blockIdx.x * ICP_NACC + tid] = v;
  }
  if (tid == 64) {
    int c = 0;
    for (int w = 0; w < 16; ++w) c += cnt[w];
    cslots[blockIdx.x] = c;
  }
}

__global__ __launch_bounds__(64) void icp_step_kernel(int it, int nslice, float tol_rot, float tol_trans, IcpState* __restrict__ st,
                                                      const double* __restrict__ slots, const int32_t* __restrict__ cslots,
                                                      double* __restrict__ trace, double* __restrict__ system) {
  __shared__ double tot[ICP_NACC];
  __shared__ long long npairs;
  const int tid = threadIdx.x;
  if (st->stop) return;
  if (tid < ICP_NACC) {
    tot[tid] = cmr_slot_sum(slots, nslice, tid);
  } else if (tid == ICP_NACC) {
    long long c = 0;
    for (int s = 0; s < nslice; ++s) c += cslots[s];
    npairs = c;
  }
  __syncthreads();
  if (system && tid < ICP_NACC) system[(int64_t)it * ICP_NACC + tid] = tot[tid];
  if (tid != 0) return;
  const long long n = npairs;
  double* tr = trace + 4 * (int64_t)it;
  st->executed = it + 1;
  tr[0] = (double)n;
  tr[1] = n > 0 ? sqrt(tot[27] / (double)n) : 0.0;
  if (n < 6) { st->code = 2; st->stop = 1; return; }
  bool ok = true;
  for (int q = 0; q < ICP_NACC; ++q) ok = ok && isfinite(tot[q]);
  double g[6], xi[6], nw[12];
  if (ok) {
    for (int r = 0; r < 6; ++r) g[r] = -tot[21 + r];
    ok = cmr_pnp_chol6<true>(tot, g, xi);
  }
  ok = ok && cmr_pose_left_update(st->cur, xi, nw);
  if (!ok) { st->code = 3; st->stop = 1; return; }                  // the pose stays the one before this iteration
  for (int i = 0; i < 12; ++i) st->cur[i] = nw[i];
  const double rot = sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]), trans = sqrt(xi[3] * xi[3] + xi[4] * xi[4] + xi[5] * xi[5]);
  tr[2] = rot;
  tr[3] = trans;
  if (rot < (double)tol_rot && trans < (double)tol_trans) { st->code = 0; st->stop = 1; }
}

__global__ __launch_bounds__(64) void icp_final_kernel(const IcpState* __restrict__ st, float* __restrict__ pose,
                                                       int32_t* __restrict__ status) {
  const int tid = threadIdx.x;
  if (tid < 16) pose[tid] = cmr_pose_entry(st->cur, tid);
  if (tid == 16) status[0] = st->code;
  if (tid == 17) status[1] = st->executed;
}

struct IcpWs { int64_t state, slots, cslots, total; };

inline int64_t icp_slices(int64_t M) { return (M + ICP_SLICE - 1) / ICP_SLICE; }
inline IcpWs icp_layout(int64_t M) {
  IcpWs L;
  L.state = 0;
  L.slots = L.state + cmr_up16(sizeof(IcpState));
  L.cslots = L.slots + cmr_up16(icp_slices(M) * ICP_NACC * 8);
  L.total = L.cslots + cmr_up16(icp_slices(M) * 4);
  return L;
}

}  // namespace

extern "C" int cmr_cloud_nearest_f32(const float* queries, int64_t ld, int64_t M, const float* pose, const float* points4,
                                     const int64_t* keys_sorted, const int64_t* order, int64_t kept, float ox, float oy, float oz,
                                     float cell, float max_dist, int32_t* idx, float* d2, hipStream_t stream) {
  const GridIndex index{(const f32x4*)points4, keys_sorted, order, kept, ox, oy, oz, cell};
  CMR_REQUIRE(queries && idx && d2 && ld >= 3 && M > 0 && M < ((int64_t)1 << 31) && grid_index_ok(index) && max_dist > 0.f && max_dist <= cell);
  hipLaunchKernelGGL(cloud_nearest_kernel, dim3((unsigned)((M + 15) / 16)), dim3(256), 0, stream, queries, ld, M, pose, index,
                     max_dist * max_dist, idx, d2);
  return cmr_launch_status();
}

extern "C" int64_t cmr_icp_point_to_plane_workspace_bytes(int64_t M) { return M > 0 ? icp_layout(M).total : 0; }

extern "C" int cmr_icp_point_to_plane_f32(const float* source, int64_t ld, int64_t M, const float* points4, const int64_t* keys_sorted,
                                          const int64_t* order, int64_t kept, float ox, float oy, float oz, float cell,
                                          const float* normals, const float* pose_in, float max_dist, float huber, int iters,
                                          float tol_rot, float tol_trans, float* pose, double* trace, double* system, int32_t* status,
                                          void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  const GridIndex index{(const f32x4*)points4, keys_sorted, order, kept, ox, oy, oz, cell};
  CMR_REQUIRE(source && normals && pose_in && pose && status && workspace && ld >= 3 && M > 0 && M < ((int64_t)1 << 31) &&
              grid_index_ok(index) && max_dist > 0.f && max_dist <= cell);
  CMR_REQUIRE(huber >= 0.f && isfinite(huber) && iters >= 0 && iters <= 1000 && (iters == 0 || trace) && tol_rot == tol_rot &&
              tol_trans == tol_trans);
  CMR_REQUIRE(cmr_aligned16(workspace) && workspace_bytes >= cmr_icp_point_to_plane_workspace_bytes(M));
  const IcpWs L = icp_layout(M);
  IcpState* st = (IcpState*)((char*)workspace + L.state);
  double* slots = (double*)((char*)workspace + L.slots);
  int32_t* cslots = (int32_t*)((char*)workspace + L.cslots);
  const int nslice = (int)icp_slices(M);
  hipLaunchKernelGGL(icp_init_kernel, dim3(1), dim3(256), 0, stream, pose_in, iters, st, trace, system);
  for (int it = 0; it < iters; ++it) {
    hipLaunchKernelGGL(icp_accum_kernel, dim3(nslice), dim3(256), 0, stream, source, ld, M, index, normals, max_dist * max_dist, huber,
                       (const IcpState*)st, slots, cslots);
    hipLaunchKernelGGL(icp_step_kernel, dim3(1), dim3(64), 0, stream, it, nslice, tol_rot, tol_trans, st, (const double*)slots,
                       (const int32_t*)cslots, trace, system);
  }
  hipLaunchKernelGGL(icp_final_kernel, dim3(1), dim3(64), 0, stream, (const IcpState*)st, pose, status);
  return cmr_launch_status();
}
