// Registration of two clouds WITHOUT a start pose (port extension): the nearest descriptor of every row, and RANSAC over
// 3-point rigid hypotheses on the correspondences that gives.  cloud_fpfh.hip supplies the descriptors, cloud_icp.hip the polish.
//
//   cmr_descriptor_nearest_f32   one launch.  A workgroup owns 64 queries, one per lane, held in registers by each of its four waves; the
//                                targets pass through LDS in tiles of 128 rows, wave w takes rows w, w + 4, ... in ascending order and every
//                                lane reads the same row (broadcast), so `d2 < best` keeps the lowest row on equal d2; the four waves' (d2,
//                                row) meet in a lexicographic minimum.  d2 is the plain fp32 sum in channel order; rows padded with zeros up
//                                to the instantiated width add + 0 * 0, which changes no bit.  Every output is a plain store.
//   cmr_ransac_rigid_f32         four launches on the caller's stream:
//     rr_pack_kernel     one workgroup: the valid rows of corr IN LIST ORDER (draws index the list) as two float4 planes, and their count;
//     rr_hyp_kernel      one lane per hypothesis: 3 hashed draws (pnp_hash of cmr_pnp.h), the edge-length and collinearity checks, the
//                        least-squares rigid transform of the three pairs in fp64 (Horn's quaternion, a 4 x 4 Jacobi eigen-solve on
//                        cmr_jacobi_rotate of cmr_common.h);
//     rr_score_kernel    a workgroup = 256 hypotheses x one 512-entry slice of the list staged in LDS; INTEGER partial counts added
//                        atomically (order free, exact);
//     rr_select_kernel   one workgroup: most inliers, ties to the lowest hypothesis; the same least squares over its inlier set, fp64 sums in
//                        a fixed order (thread t adds entries t, t + 256, ..., then a tree over the threads); recount; outputs (the
//                        pose's fp32 4x4 form is cmr_pose_entry of cmr_pnp.h).
#include "cmr_cloud_grid.h"
#include "cmr_pnp.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------- descriptor nearest
constexpr int DN_QUERIES = 64;       // queries per workgroup: one per lane, the same 64 in each of the four waves
constexpr int DN_WAVES = 4;          // wave w takes the rows w, w + 4, ... of every tile
constexpr int DN_THREADS = DN_QUERIES * DN_WAVES;
constexpr int DN_TILE = 128;

// acc = acc + (q_c - t_c) (q_c - t_c) over the CP channels of one LDS row, in order
template <int CP>
__device__ __forceinline__ float desc_d2(const float (&q)[CP], const float* __restrict__ row) {
#pragma clang fp contract(off)
  const f32x4* t = reinterpret_cast<const f32x4*>(row);
  float acc = 0.f;
#pragma unroll
  for (int c4 = 0; c4 < CP / 4; ++c4) {
    const f32x4 v = t[c4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float d = q[4 * c4 + u] - v[u];
      acc = acc + d * d;
    }
  }
  return acc;
}

template <int CP>
__global__ __launch_bounds__(DN_THREADS) void desc_nearest_kernel(const float* __restrict__ queries, int64_t M, const float* __restrict__ targets,
                                                                   int64_t N, int C, const uint8_t* __restrict__ qmask,
                                                                   const uint8_t* __restrict__ tmask, int32_t* __restrict__ idx,
                                                                   float* __restrict__ d2out) {
  __shared__ __attribute__((aligned(16))) float tile[DN_TILE * CP];
  __shared__ int sel[DN_TILE];
  __shared__ float wbest[DN_WAVES][DN_QUERIES];
  __shared__ int wrow[DN_WAVES][DN_QUERIES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t i = (int64_t)blockIdx.x * DN_QUERIES + lane;
  const bool have = i < M;
  float q[CP];
  bool ok = have && (!qmask || qmask[i] != 0);
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    q[c] = have && c < C ? queries[i * C + c] : 0.f;
    ok = ok && isfinite(q[c]);
  }
  float best = INFINITY;
  int row = INT32_MAX;
  for (int64_t base = 0; base < N; base += DN_TILE) {
    const int rows = N - base < DN_TILE ? (int)(N - base) : DN_TILE;
    __syncthreads();                                                // the tile before this one has been read
    for (int e = tid; e < DN_TILE * CP; e += DN_THREADS) {
      const int r = e / CP, c = e - r * CP;
      tile[e] = r < rows && c < C ? targets[(base + r) * C + c] : 0.f;
    }
    if (tid < DN_TILE) sel[tid] = tid < rows && (!tmask || tmask[base + tid] != 0);
    __syncthreads();
    // two rows at a time, two independent chains of additions; taken in ascending order, so `<` keeps the lower row on equal d2.  A row
    // past the tile's end is zeros and unselected.
    for (int r = wave; r < rows; r += 2 * DN_WAVES) {
      const float a0 = desc_d2<CP>(q, tile + r * CP), a1 = desc_d2<CP>(q, tile + (r + DN_WAVES) * CP);
      if (sel[r] && a0 < best) {                                    // sel is uniform over the wave; never true for a NaN or an infinite d2
        best = a0;
        row = (int)(base + r);
      }
      if (sel[r + DN_WAVES] && a1 < best) {
        best = a1;
        row = (int)(base + r + DN_WAVES);
      }
    }
  }
  // the four waves' least (d2, row) of a query, lexicographically: the result does not depend on which wave met which row
  wbest[wave][lane] = best;
  wrow[wave][lane] = row;
  __syncthreads();
  if (wave != 0 || !have) return;
#pragma unroll
  for (int w = 1; w < DN_WAVES; ++w) {
    const float ob = wbest[w][lane];
    const int orow = wrow[w][lane];
    if (ob < best || (ob == best && orow < row)) {
      best = ob;
      row = orow;
    }
  }
  const bool found = ok && row != INT32_MAX;
  idx[i] = found ? row : -1;
  d2out[i] = found ? best : NAN;
}

// ------------------------------------------------------------------------------------------------------------------------------ RANSAC
constexpr int RR_PACK_THREADS = 1024;
constexpr int RR_SLICE = 512;        // list entries per scoring workgroup
constexpr int RR_HYP_WG = 256;       // hypotheses per scoring workgroup
constexpr int RR_SEL_THREADS = 256;  // a constant: the summation order of the refit rests on it
constexpr int RR_MAX_DRAWS = 32;     // hash counters a hypothesis may use for its 3 distinct draws
constexpr int RR_JACOBI_SWEEPS = 10; // cyclic Jacobi on a 4 x 4 in fp64: six sweeps reach the last bit, ten are fixed
constexpr double RR_COLLINEAR = 1e-4;  // a triple is collinear when sin^2 of the angle at its first point is at most this, on either side

// The valid rows of corr in list order.  One workgroup walks the list 1024 rows at a time: ballot ranks inside a wave, the 16 wave counts
// through LDS.
__global__ __launch_bounds__(RR_PACK_THREADS) void rr_pack_kernel(const float* __restrict__ src, int64_t M, const float* __restrict__ tgt,
                                                                  int64_t N, const int32_t* __restrict__ corr, int L, f32x4* __restrict__ la,
                                                                  f32x4* __restrict__ lb, int32_t* __restrict__ cnt) {
  __shared__ int wc[RR_PACK_THREADS / 64];
  const int tid = threadIdx.x, wave = tid >> 6, wl = tid & 63;
  int done = 0;
  for (int base = 0; base < L; base += RR_PACK_THREADS) {
    const int r = base + tid;
    bool ok = false;
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
    if (r < L) {
      const int s = corr[2 * (int64_t)r], t = corr[2 * (int64_t)r + 1];
      if (s >= 0 && s < M && t >= 0 && t < N) {
        a = f32x4{src[3 * (int64_t)s], src[3 * (int64_t)s + 1], src[3 * (int64_t)s + 2], 0.f};
        b = f32x4{tgt[3 * (int64_t)t], tgt[3 * (int64_t)t + 1], tgt[3 * (int64_t)t + 2], 0.f};
        ok = cmr_finite3(a.x, a.y, a.z) && cmr_finite3(b.x, b.y, b.z);
      }
    }
    const unsigned long long bal = __ballot(ok);
    if (wl == 0) wc[wave] = __popcll(bal);
    __syncthreads();
    int before = done, total = done;
    for (int w = 0; w < RR_PACK_THREADS / 64; ++w) {
      before += w < wave ? wc[w] : 0;
      total += wc[w];
    }
    if (ok) {
      const int at = before + __popcll(bal & ((1ull << wl) - 1ull));
      la[at] = a;
      lb[at] = b;
    }
    done = total;
    __syncthreads();
  }
  if (tid == 0) cnt[0] = done;
}

struct V3d { double x, y, z; };
__device__ __forceinline__ V3d v3d(const f32x4& p) { return V3d{(double)p.x, (double)p.y, (double)p.z}; }
__device__ __forceinline__ V3d sub(const V3d& a, const V3d& b) { return V3d{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dot(const V3d& a, const V3d& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3d cross(const V3d& a, const V3d& b) { return V3d{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// The rotation R (row-major) maximising trace(R S^T) over det R = +1 for S = sum a b^T (centred), i.e. minimising sum |R a - b|^2: Horn's
// unit quaternion, the eigenvector of the largest eigenvalue of a symmetric 4 x 4.  Proper for a rank-2 S (three pairs) as for a full one.
__device__ void rr_rotation(const double (&S)[3][3], double (&R)[9]) {
  double a[4][4], v[4][4];
  a[0][0] = S[0][0] + S[1][1] + S[2][2];
  a[1][1] = S[0][0] - S[1][1] - S[2][2];
  a[2][2] = -S[0][0] + S[1][1] - S[2][2];
  a[3][3] = -S[0][0] - S[1][1] + S[2][2];
  a[0][1] = a[1][0] = S[1][2] - S[2][1];
  a[0][2] = a[2][0] = S[2][0] - S[0][2];
  a[0][3] = a[3][0] = S[0][1] - S[1][0];
  a[1][2] = a[2][1] = S[0][1] + S[1][0];
  a[1][3] = a[3][1] = S[2][0] + S[0][2];
  a[2][3] = a[3][2] = S[1][2] + S[2][1];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) v[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < RR_JACOBI_SWEEPS; ++sweep) {
    cmr_jacobi_rotate<0, 1>(a, v);
    cmr_jacobi_rotate<0, 2>(a, v);
    cmr_jacobi_rotate<0, 3>(a, v);
    cmr_jacobi_rotate<1, 2>(a, v);
    cmr_jacobi_rotate<1, 3>(a, v);
    cmr_jacobi_rotate<2, 3>(a, v);
  }
  double qw = v[0][0], qx = v[1][0], qy = v[2][0], qz = v[3][0], top = a[0][0];
#pragma unroll
  for (int c = 1; c < 4; ++c)
    if (a[c][c] > top) {
      top = a[c][c];
      qw = v[0][c], qx = v[1][c], qy = v[2][c], qz = v[3][c];
    }
  const double n = 1.0 / sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
  qw *= n, qx *= n, qy *= n, qz *= n;
  R[0] = 1.0 - 2.0 * (qy * qy + qz * qz);
  R[1] = 2.0 * (qx * qy - qw * qz);
  R[2] = 2.0 * (qx * qz + qw * qy);
  R[3] = 2.0 * (qx * qy + qw * qz);
  R[4] = 1.0 - 2.0 * (qx * qx + qz * qz);
  R[5] = 2.0 * (qy * qz - qw * qx);
  R[6] = 2.0 * (qx * qz - qw * qy);
  R[7] = 2.0 * (qy * qz + qw * qx);
  R[8] = 1.0 - 2.0 * (qx * qx + qy * qy);
}
// pose = [R | t] with t = mean b - R mean a
__device__ __forceinline__ void rr_pose(const double (&S)[3][3], const V3d& ma, const V3d& mb, double* pose) {
  double R[9];
  rr_rotation(S, R);
  for (int i = 0; i < 9; ++i) pose[i] = R[i];
  pose[9] = mb.x - ((R[0] * ma.x + R[1] * ma.y) + R[2] * ma.z);
  pose[10] = mb.y - ((R[3] * ma.x + R[4] * ma.y) + R[5] * ma.z);
  pose[11] = mb.z - ((R[6] * ma.x + R[7] * ma.y) + R[8] * ma.z);
}
// the inlier test: |R a + t - b|^2 <= thr^2 in fp64
__device__ __forceinline__ bool rr_inlier(const double* T, const f32x4& a, const f32x4& b, double thr2) {
  const double ax = a.x, ay = a.y, az = a.z;
  const double rx = (((T[0] * ax + T[1] * ay) + T[2] * az) + T[9]) - (double)b.x;
  const double ry = (((T[3] * ax + T[4] * ay) + T[5] * az) + T[10]) - (double)b.y;
  const double rz = (((T[6] * ax + T[7] * ay) + T[8] * az) + T[11]) - (double)b.z;
  return (rx * rx + ry * ry) + rz * rz <= thr2;
}

__global__ __launch_bounds__(64) void rr_hyp_kernel(const f32x4* __restrict__ la, const f32x4* __restrict__ lb, const int32_t* __restrict__ cnt,
                                                    int n_hyp, uint32_t seed, float edge_ratio, double* __restrict__ hyp_pose,
                                                    int32_t* __restrict__ hyp_inl) {
  const int h = blockIdx.x * 64 + threadIdx.x;
  if (h >= n_hyp) return;
  const int count = cnt[0];
  int idx[3], got = 0;
  if (count >= 3) {
    for (uint32_t c = 0; c < RR_MAX_DRAWS && got < 3; ++c) {
      const int i = (int)(pnp_hash(seed, 0u, (uint32_t)h, c) % (uint32_t)count);
      bool dup = false;
      for (int k = 0; k < got; ++k) dup |= idx[k] == i;
      if (!dup) idx[got++] = i;
    }
  }
  bool ok = got == 3;
  double pose[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  if (ok) {
    V3d a[3], b[3];
    for (int k = 0; k < 3; ++k) {
      a[k] = v3d(la[idx[k]]);
      b[k] = v3d(lb[idx[k]]);
    }
    const double ratio = (double)edge_ratio;
    for (int k = 0; k < 3; ++k) {                                   // edges 0-1, 1-2, 2-0
      const V3d ea = sub(a[(k + 1) % 3], a[k]), eb = sub(b[(k + 1) % 3], b[k]);
      const double da = sqrt(dot(ea, ea)), db = sqrt(dot(eb, eb));
      ok = ok && !(fmin(da, db) < ratio * fmax(da, db));
    }
    const V3d a1 = sub(a[1], a[0]), a2 = sub(a[2], a[0]), b1 = sub(b[1], b[0]), b2 = sub(b[2], b[0]);
    const V3d ca = cross(a1, a2), cb = cross(b1, b2);
    ok = ok && dot(ca, ca) > RR_COLLINEAR * (dot(a1, a1) * dot(a2, a2)) && dot(cb, cb) > RR_COLLINEAR * (dot(b1, b1) * dot(b2, b2));
    if (ok) {
      const V3d ma = {((a[0].x + a[1].x) + a[2].x) / 3.0, ((a[0].y + a[1].y) + a[2].y) / 3.0, ((a[0].z + a[1].z) + a[2].z) / 3.0};
      const V3d mb = {((b[0].x + b[1].x) + b[2].x) / 3.0, ((b[0].y + b[1].y) + b[2].y) / 3.0, ((b[0].z + b[1].z) + b[2].z) / 3.0};
      double S[3][3] = {};
      for (int k = 0; k < 3; ++k) {
        const V3d x = sub(a[k], ma), y = sub(b[k], mb);
        S[0][0] += x.x * y.x, S[0][1] += x.x * y.y, S[0][2] += x.x * y.z;
        S[1][0] += x.y * y.x, S[1][1] += x.y * y.y, S[1][2] += x.y * y.z;
        S[2][0] += x.z * y.x, S[2][1] += x.z * y.y, S[2][2] += x.z * y.z;
      }
      rr_pose(S, ma, mb, pose);
      for (int i = 0; i < 12; ++i) ok = ok && isfinite(pose[i]);
    }
  }
  for (int i = 0; i < 12; ++i) hyp_pose[(int64_t)h * 12 + i] = pose[i];
  hyp_inl[h] = ok ? 0 : -1;
}

__global__ __launch_bounds__(RR_HYP_WG) void rr_score_kernel(const f32x4* __restrict__ la, const f32x4* __restrict__ lb,
                                                             const int32_t* __restrict__ cnt, int n_hyp, float thr,
                                                             const double* __restrict__ hyp_pose, int32_t* __restrict__ hyp_inl) {
  __shared__ f32x4 sa[RR_SLICE], sb[RR_SLICE];
  const int count = cnt[0];
  const int first = blockIdx.y * RR_SLICE;
  if (first >= count) return;                                       // uniform over the workgroup
  const int n = count - first < RR_SLICE ? count - first : RR_SLICE;
  for (int e = threadIdx.x; e < n; e += RR_HYP_WG) {
    sa[e] = la[first + e];
    sb[e] = lb[first + e];
  }
  __syncthreads();
  const int h = blockIdx.x * RR_HYP_WG + threadIdx.x;
  if (h >= n_hyp || hyp_inl[h] < 0) return;                         // an invalid hypothesis keeps its -1: nobody adds to it
  double T[12];
  for (int i = 0; i < 12; ++i) T[i] = hyp_pose[(int64_t)h * 12 + i];
  const double thr2 = (double)thr * (double)thr;
  int c = 0;
  for (int e = 0; e < n; ++e) c += rr_inlier(T, sa[e], sb[e], thr2) ? 1 : 0;
  if (c) atomicAdd(&hyp_inl[h], c);
}

// the sum of v over the workgroup in a fixed order, valid in every thread: a tree over the threads in LDS
template <typename T>
__device__ __forceinline__ T rr_block_sum(T v, T* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = RR_SEL_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(RR_SEL_THREADS) void rr_select_kernel(const f32x4* __restrict__ la, const f32x4* __restrict__ lb,
                                                                   const int32_t* __restrict__ cnt, int n_hyp, float thr,
                                                                   const double* __restrict__ hyp_pose, const int32_t* __restrict__ hyp_inl,
                                                                   float* __restrict__ pose_out, int32_t* __restrict__ out3) {
  __shared__ double red[RR_SEL_THREADS];
  __shared__ int ired[RR_SEL_THREADS];
  __shared__ int bi[RR_SEL_THREADS], bh[RR_SEL_THREADS];
  __shared__ double refit[12];
  __shared__ int keep;
  const int tid = threadIdx.x;
  const int count = cnt[0];
  // most inliers, ties to the lowest hypothesis
  int mi = -1, mh = INT32_MAX;
  for (int h = tid; h < n_hyp; h += RR_SEL_THREADS) {
    const int v = hyp_inl[h];
    if (v > mi) {
      mi = v;
      mh = h;
    }
  }
  bi[tid] = mi;
  bh[tid] = mh;
  __syncthreads();
  for (int o = RR_SEL_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o && (bi[tid + o] > bi[tid] || (bi[tid + o] == bi[tid] && bh[tid + o] < bh[tid]))) {
      bi[tid] = bi[tid + o];
      bh[tid] = bh[tid + o];
    }
    __syncthreads();
  }
  const int best_inl = bi[0], best = bh[0];
  if (count < 3 || best_inl < 0) {                                  // uniform over the workgroup
    if (tid < 16) pose_out[tid] = (tid >> 2) == (tid & 3) ? 1.f : 0.f;
    if (tid == 16) out3[0] = 0;
    if (tid == 17) out3[1] = count < 3 ? 1 : 2;
    if (tid == 18) out3[2] = -1;
    return;
  }
  double T[12];
  for (int i = 0; i < 12; ++i) T[i] = hyp_pose[(int64_t)best * 12 + i];
  const double thr2 = (double)thr * (double)thr;
  // the refit over the inlier set: means, then the centred cross-covariance
  double s[7] = {};
  for (int e = tid; e < count; e += RR_SEL_THREADS) {
    const f32x4 a = la[e], b = lb[e];
    if (rr_inlier(T, a, b, thr2)) {
      s[0] += 1.0;
      s[1] += (double)a.x, s[2] += (double)a.y, s[3] += (double)a.z;
      s[4] += (double)b.x, s[5] += (double)b.y, s[6] += (double)b.z;
    }
  }
  for (int i = 0; i < 7; ++i) s[i] = rr_block_sum(s[i], red);
  const V3d ma = {s[1] / s[0], s[2] / s[0], s[3] / s[0]}, mb = {s[4] / s[0], s[5] / s[0], s[6] / s[0]};
  double c[9] = {};
  for (int e = tid; e < count; e += RR_SEL_THREADS) {
    const f32x4 a = la[e], b = lb[e];
    if (rr_inlier(T, a, b, thr2)) {
      const V3d x = sub(v3d(a), ma), y = sub(v3d(b), mb);
      c[0] += x.x * y.x, c[1] += x.x * y.y, c[2] += x.x * y.z;
      c[3] += x.y * y.x, c[4] += x.y * y.y, c[5] += x.y * y.z;
      c[6] += x.z * y.x, c[7] += x.z * y.y, c[8] += x.z * y.z;
    }
  }
  for (int i = 0; i < 9; ++i) c[i] = rr_block_sum(c[i], red);
  if (tid == 0) {
    const double S[3][3] = {{c[0], c[1], c[2]}, {c[3], c[4], c[5]}, {c[6], c[7], c[8]}};
    double P[12];
    rr_pose(S, ma, mb, P);
    bool fin = true;
    for (int i = 0; i < 12; ++i) {
      fin = fin && isfinite(P[i]);
      refit[i] = P[i];
    }
    keep = fin ? 1 : 0;
  }
  __syncthreads();
  double Tn[12];
  for (int i = 0; i < 12; ++i) Tn[i] = refit[i];
  int again = 0;
  if (keep)                                                         // uniform: LDS
    for (int e = tid; e < count; e += RR_SEL_THREADS) again += rr_inlier(Tn, la[e], lb[e], thr2) ? 1 : 0;
  again = rr_block_sum(again, ired);
  const bool take = keep && again >= best_inl;                      // the refit is kept if the count does not drop
  if (tid < 16) pose_out[tid] = cmr_pose_entry(take ? Tn : T, tid);
  if (tid == 16) out3[0] = take ? again : best_inl;
  if (tid == 17) out3[1] = 0;
  if (tid == 18) out3[2] = best;
}

struct RrWs { int64_t la, lb, cnt, pose, inl, total; };
inline RrWs rr_layout(int64_t L, int n_hyp) {
  RrWs W;
  W.la = 0;
  W.lb = W.la + cmr_up16(L * 16);
  W.cnt = W.lb + cmr_up16(L * 16);
  W.pose = W.cnt + 16;
  W.inl = W.pose + cmr_up16((int64_t)n_hyp * 12 * 8);
  W.total = W.inl + cmr_up16((int64_t)n_hyp * 4);
  return W;
}

template <int CP>
void desc_launch(const float* q, int64_t M, const float* t, int64_t N, int C, const uint8_t* qm, const uint8_t* tm, int32_t* idx, float* d2,
                 hipStream_t stream) {
  hipLaunchKernelGGL(desc_nearest_kernel<CP>, dim3((unsigned)((M + DN_QUERIES - 1) / DN_QUERIES)), dim3(DN_THREADS), 0, stream, q, M, t, N, C, qm,
                     tm, idx, d2);
}

}  // namespace

extern "C" int cmr_descriptor_nearest_f32(const float* queries, int64_t M, const float* targets, int64_t N, int C, const void* query_mask,
                                          const void* target_mask, int32_t* idx, float* d2, hipStream_t stream) {
  CMR_REQUIRE(queries && targets && idx && d2 && M > 0 && M < ((int64_t)1 << 31) && N > 0 && N < ((int64_t)1 << 31) && C > 0);
  if (C > 64) return CMR_EUNSUPPORTED;
  const uint8_t* qm = (const uint8_t*)query_mask;
  const uint8_t* tm = (const uint8_t*)target_mask;
  if (C <= 4) desc_launch<4>(queries, M, targets, N, C, qm, tm, idx, d2, stream);
  else if (C <= 16) desc_launch<16>(queries, M, targets, N, C, qm, tm, idx, d2, stream);
  else if (C <= 36) desc_launch<36>(queries, M, targets, N, C, qm, tm, idx, d2, stream);
  else desc_launch<64>(queries, M, targets, N, C, qm, tm, idx, d2, stream);
  return cmr_launch_status();
}

extern "C" int64_t cmr_ransac_rigid_workspace_bytes(int64_t L, int n_hyp) { return L > 0 && n_hyp > 0 ? rr_layout(L, n_hyp).total : 0; }

extern "C" int cmr_ransac_rigid_f32(const float* source, int64_t M, const float* target, int64_t N, const int32_t* corr, int64_t L, int n_hyp,
                                    float thr, float edge_ratio, uint32_t seed, float* pose, int32_t* result, int32_t* hyp_inliers,
                                    void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  CMR_REQUIRE(source && target && corr && pose && result && workspace && cmr_aligned16(workspace) && M > 0 && M < ((int64_t)1 << 31) && N > 0 &&
              N < ((int64_t)1 << 31) && L > 0 && L <= ((int64_t)1 << 24) && n_hyp > 0 && n_hyp <= (1 << 20));
  CMR_REQUIRE(thr > 0.f && isfinite(thr) && edge_ratio >= 0.f && edge_ratio <= 1.f &&
              workspace_bytes >= cmr_ransac_rigid_workspace_bytes(L, n_hyp));
  const RrWs W = rr_layout(L, n_hyp);
  char* ws = (char*)workspace;
  f32x4* la = (f32x4*)(ws + W.la);
  f32x4* lb = (f32x4*)(ws + W.lb);
  int32_t* cnt = (int32_t*)(ws + W.cnt);
  double* hyp_pose = (double*)(ws + W.pose);
  int32_t* hyp_inl = hyp_inliers ? hyp_inliers : (int32_t*)(ws + W.inl);
  hipLaunchKernelGGL(rr_pack_kernel, dim3(1), dim3(RR_PACK_THREADS), 0, stream, source, M, target, N, corr, (int)L, la, lb, cnt);
  hipLaunchKernelGGL(rr_hyp_kernel, dim3((unsigned)((n_hyp + 63) / 64)), dim3(64), 0, stream, (const f32x4*)la, (const f32x4*)lb,
                     (const int32_t*)cnt, n_hyp, seed, edge_ratio, hyp_pose, hyp_inl);
  hipLaunchKernelGGL(rr_score_kernel, dim3((unsigned)((n_hyp + RR_HYP_WG - 1) / RR_HYP_WG), (unsigned)((L + RR_SLICE - 1) / RR_SLICE)),
                     dim3(RR_HYP_WG), 0, stream, (const f32x4*)la, (const f32x4*)lb, (const int32_t*)cnt, n_hyp, thr,
                     (const double*)hyp_pose, hyp_inl);
  hipLaunchKernelGGL(rr_select_kernel, dim3(1), dim3(RR_SEL_THREADS), 0, stream, (const f32x4*)la, (const f32x4*)lb, (const int32_t*)cnt, n_hyp,
                     thr, (const double*)hyp_pose, (const int32_t*)hyp_inl, pose, result);
  return cmr_launch_status();
}
