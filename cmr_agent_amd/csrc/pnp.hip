// Camera pose from 2-D/3-D correspondences: PnP inside RANSAC.  Every sample of the batch is solved on its own; the
// correspondence count of a sample is read on the device, so the whole call is graph-capturable.
//
// Five launches, all on the caller's stream (plus one memset of the hypothesis counts):
//   pnp_chunk_count_kernel  selected rows per 256-row chunk of every sample;
//   pnp_pack_kernel         the selected rows in row order (prefix over the chunk counts, then ballot ranks inside the chunk) packed
//                           as five planes X, Y, Z, u, v, and the sample's count;
//   pnp_hyp_kernel          one lane per (sample, hypothesis): 4 hashed draws, Lambda Twist P3P in float64 on the first three, the
//                           fourth point picks among the up to four solutions; the 3x4 matrix K[R|t] in fp32 for scoring;
//   pnp_score_kernel        a workgroup = 256 hypotheses x one 512-entry slice of the correspondence list, the slice staged in LDS and
//                           read as broadcasts; integer partial counts added atomically (order free);
//   pnp_select_kernel       one workgroup per sample: most inliers (ties to the lowest hypothesis index), Gauss-Newton on that
//                           hypothesis' inlier set in float64, inlier recount, output.  A correspondence's terms, the left update of
//                           the pose and its fp32 4x4 form are cmr_pnp.h's, shared with pnp_refine.hip and cloud_icp.hip.
// The row order of the list is kept (not fm_compact_kernel's atomic order): draws index the list, so its order is part of the result.
#include "cmr_pnp.h"

namespace {

constexpr int PNP_CHUNK = 256;       // rows per compaction workgroup
constexpr int PNP_SLICE = 512;       // list entries per scoring workgroup
constexpr int PNP_HYP_WG = 256;      // hypotheses per scoring workgroup
constexpr int PNP_SEL_THREADS = 1024;
constexpr int PNP_MAX_DRAWS = 32;    // hash counters a hypothesis may use for its 4 distinct draws
constexpr int PNP_NACC = CMR_GN_NACC; // J^T J (21 upper-triangle entries), J^T r (6), cost
constexpr double PNP_ORTH_TOL = 1e-5;  // a P3P solution is kept only if max |R R^T - I| <= this

// ---- hash: pnp_hash, stated once in cmr_pnp.h (cloud_global.hip draws its hypotheses with it too) ------------------------------------

// ---- compaction ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PNP_CHUNK) void pnp_chunk_count_kernel(const void* __restrict__ mask, int mask_bytes, int N, int nchunk,
                                                                    int32_t* __restrict__ chunk_cnt) {
  __shared__ int wc[PNP_CHUNK / 64];
  const int b = blockIdx.y, n = blockIdx.x * PNP_CHUNK + threadIdx.x;
  const bool sel = n < N && cmr_sel(mask, mask_bytes, (int64_t)b * N + n);
  const int c = __popcll(__ballot(sel));
  if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) chunk_cnt[(int64_t)b * nchunk + blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

__global__ __launch_bounds__(PNP_CHUNK) void pnp_pack_kernel(const float* __restrict__ pts, const float* __restrict__ uv,
                                                             const void* __restrict__ mask, int mask_bytes, int N, int nchunk,
                                                             const int32_t* __restrict__ chunk_cnt, float* __restrict__ corr,
                                                             int32_t* __restrict__ count) {
  __shared__ int red[PNP_CHUNK];
  __shared__ int wc[PNP_CHUNK / 64];
  const int b = blockIdx.y, c = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int s = 0;
  for (int i = threadIdx.x; i < c; i += PNP_CHUNK) s += chunk_cnt[(int64_t)b * nchunk + i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int k = PNP_CHUNK / 2; k > 0; k >>= 1) {
    if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  const int base = red[0];
  const int n = c * PNP_CHUNK + threadIdx.x;
  const bool sel = n < N && cmr_sel(mask, mask_bytes, (int64_t)b * N + n);
  const unsigned long long bal = __ballot(sel);
  if (lane == 0) wc[wave] = __popcll(bal);
  __syncthreads();
  int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) pos += wc[w];
  if (sel) {
    float* dst = corr + (int64_t)b * 5 * N;
    const float* p = pts + (int64_t)b * 3 * N;
    const float* q = uv + (int64_t)b * 2 * N;
    dst[pos] = p[n];
    dst[N + pos] = p[N + n];
    dst[2 * N + pos] = p[2 * N + n];
    dst[3 * N + pos] = q[n];
    dst[4 * N + pos] = q[N + n];
  }
  if (c == nchunk - 1 && threadIdx.x == 0) count[b] = base + wc[0] + wc[1] + wc[2] + wc[3];
}

// ---- float64 3-vector / 3x3 helpers (row-major) ----------------------------------------------------------------------------------
struct V3 { double x, y, z; };
__device__ __forceinline__ V3 v3(double x, double y, double z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 scl(V3 a, double s) { return v3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
__device__ __forceinline__ V3 mulv(const double* A, V3 x) {
  return v3(A[0] * x.x + A[1] * x.y + A[2] * x.z, A[3] * x.x + A[4] * x.y + A[5] * x.z, A[6] * x.x + A[7] * x.y + A[8] * x.z);
}
__device__ __forceinline__ double det3(const double* A) {
  return A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]);
}
// adjugate (transpose of the cofactor matrix): A adj(A) = det(A) I
__device__ __forceinline__ void adj3(const double* A, double* J) {
  J[0] = A[4] * A[8] - A[5] * A[7]; J[1] = A[2] * A[7] - A[1] * A[8]; J[2] = A[1] * A[5] - A[2] * A[4];
  J[3] = A[5] * A[6] - A[3] * A[8]; J[4] = A[0] * A[8] - A[2] * A[6]; J[5] = A[2] * A[3] - A[0] * A[5];
  J[6] = A[3] * A[7] - A[4] * A[6]; J[7] = A[1] * A[6] - A[0] * A[7]; J[8] = A[0] * A[4] - A[1] * A[3];
}
__device__ __forceinline__ double tr_mul(const double* A, const double* B) {     // trace(A B)
  double s = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) s += A[3 * i + k] * B[3 * k + i];
  return s;
}

// real roots of c3 g^3 + c2 g^2 + c1 g + c0 (c3 != 0), each polished by two Newton steps; -> number of roots (1 or 3)
__device__ int pnp_cubic(double c3, double c2, double c1, double c0, double* r) {
  const double a = c2 / c3, b = c1 / c3, c = c0 / c3;
  const double p = b - a * a / 3.0, q = 2.0 * a * a * a / 27.0 - a * b / 3.0 + c;
  const double disc = q * q / 4.0 + p * p * p / 27.0;
  int n;
  if (disc > 0.0) {
    const double sd = sqrt(disc);
    r[0] = cbrt(-q / 2.0 + sd) + cbrt(-q / 2.0 - sd) - a / 3.0;
    n = 1;
  } else {
    const double m = sqrt(fmax(-p / 3.0, 0.0));
    const double arg = m > 0.0 ? fmin(fmax(-q / (2.0 * m * m * m), -1.0), 1.0) : 0.0;
    const double phi = acos(arg) / 3.0;
    for (int k = 0; k < 3; ++k) r[k] = 2.0 * m * cos(phi - 2.0943951023931957 * k) - a / 3.0;
    n = 3;
  }
  for (int k = 0; k < n; ++k)
    for (int it = 0; it < 2; ++it) {
      const double g = r[k];
      const double f = ((c3 * g + c2) * g + c1) * g + c0, d = (3.0 * c3 * g + 2.0 * c2) * g + c1;
      if (d != 0.0) r[k] = g - f / d;
    }
  return n;
}

// unit eigenvector of the symmetric A for eigenvalue s: the largest cross product of two rows of A - s I
__device__ V3 pnp_eigvec(const double* A, double s) {
  const V3 r0 = v3(A[0] - s, A[1], A[2]), r1 = v3(A[3], A[4] - s, A[5]), r2 = v3(A[6], A[7], A[8] - s);
  V3 e = cross(r0, r1);
  double best = dot(e, e);
  const V3 c02 = cross(r0, r2), c12 = cross(r1, r2);
  if (dot(c02, c02) > best) { e = c02; best = dot(c02, c02); }
  if (dot(c12, c12) > best) { e = c12; best = dot(c12, c12); }
  return scl(e, 1.0 / sqrt(best));
}

// Lambda Twist P3P (Persson & Nordberg, ECCV 2018): x_i world points, y_i unit bearings.  Writes up to 4 (R, t) with
// lambda_i y_i = R x_i + t, lambda_i > 0; -> count.
__device__ int pnp_p3p(const V3* x, const V3* y, double (*Rs)[9], V3* ts) {
  const V3 d12 = sub(x[0], x[1]), d13 = sub(x[0], x[2]), d23 = sub(x[1], x[2]);
  const V3 n123 = cross(d12, d13);
  const double a12 = dot(d12, d12), a13 = dot(d13, d13), a23 = dot(d23, d23);
  if (!(dot(n123, n123) > 1e-10 * a12 * a13)) return 0;                  // coincident or collinear
  const double b12 = dot(y[0], y[1]), b13 = dot(y[0], y[2]), b23 = dot(y[1], y[2]);
  // Lambda^T M_ij Lambda = a_ij; D1 = a23 M12 - a12 M23, D2 = a23 M13 - a13 M23 vanish on the solution
  const double D1[9] = {a23, -a23 * b12, 0.0, -a23 * b12, a23 - a12, a12 * b23, 0.0, a12 * b23, -a12};
  const double D2[9] = {a23, 0.0, -a23 * b13, 0.0, -a13, a13 * b23, -a23 * b13, a13 * b23, a23 - a13};
  double J1[9], J2[9];
  adj3(D1, J1);
  adj3(D2, J2);
  const double c3 = det3(D2), c2 = tr_mul(J2, D1), c1 = tr_mul(J1, D2), c0 = det3(D1);   // det(D1 + g D2)
  if (!(c3 != 0.0) || !isfinite(c3 + c2 + c1 + c0)) return 0;
  double roots[3];
  const int nr = pnp_cubic(c3, c2, c1, c0, roots);
  // the degenerate member D0 = D1 + g D2 that splits into two real planes: nonzero eigenvalues of opposite sign (minor sum < 0),
  // the most balanced pair -m / (s1^2 + s2^2) wins, the first root on a tie
  double D0[9], bestq = 0.0, s1 = 0.0, s2 = 0.0;
  int pick = -1;
  for (int k = 0; k < nr; ++k) {
    const double g = roots[k];
    double A[9];
    for (int i = 0; i < 9; ++i) A[i] = D1[i] + g * D2[i];
    const double tr = A[0] + A[4] + A[8];
    const double m = (A[0] * A[4] - A[1] * A[3]) + (A[0] * A[8] - A[2] * A[6]) + (A[4] * A[8] - A[5] * A[7]);
    const double disc = tr * tr - 4.0 * m;
    if (!(m < 0.0) || !(disc >= 0.0)) continue;
    const double sq = sqrt(disc);
    const double ea = 0.5 * (tr + sq), eb = 0.5 * (tr - sq);
    const double q = -m / (ea * ea + eb * eb);
    if (q > bestq) {
      bestq = q;
      pick = k;
      for (int i = 0; i < 9; ++i) D0[i] = A[i];
      if (fabs(ea) >= fabs(eb)) { s1 = ea; s2 = eb; } else { s1 = eb; s2 = ea; }
    }
  }
  if (pick < 0) return 0;
  const V3 e1 = pnp_eigvec(D0, s1), e2 = pnp_eigvec(D0, s2);
  const double s = sqrt(-s2 / s1);
  const double X[9] = {d12.x, d13.x, n123.x, d12.y, d13.y, n123.y, d12.z, d13.z, n123.z};
  double Xi[9];
  adj3(X, Xi);
  const double dx = det3(X);
  for (int i = 0; i < 9; ++i) Xi[i] /= dx;
  int ns = 0;
  for (int sg = 0; sg < 2; ++sg) {
    const double ss = sg == 0 ? s : -s;
    const V3 n = sub(e1, scl(e2, ss));                                 // plane n . Lambda = 0
    if (!(fabs(n.x) > 1e-12 * sqrt(dot(n, n)))) continue;
    const double w0 = -n.y / n.x, w1 = -n.z / n.x;                     // lambda1 = w0 lambda2 + w1 lambda3
    // a13 (M12 form) - a12 (M13 form) = 0 with Lambda = lambda2 (w0 + w1 tau, 1, tau)
    const double qa = (a13 - a12) * w1 * w1 + 2.0 * a12 * b13 * w1 - a12;
    const double qb = 2.0 * ((a13 - a12) * w0 * w1 - a13 * b12 * w1 + a12 * b13 * w0);
    const double qc = (a13 - a12) * w0 * w0 - 2.0 * a13 * b12 * w0 + a13;
    const double disc = qb * qb - 4.0 * qa * qc;
    if (!(qa != 0.0) || !(disc >= 0.0)) continue;
    const double qq = -0.5 * (qb + copysign(sqrt(disc), qb));
    const double taus[2] = {qq / qa, qq != 0.0 ? qc / qq : 0.0};
    for (int k = 0; k < 2; ++k) {
      const double tau = taus[k];
      if (!(tau > 0.0)) continue;
      const double den = tau * tau - 2.0 * b23 * tau + 1.0;
      if (!(den > 0.0)) continue;
      const double l2 = sqrt(a23 / den), l3 = tau * l2, l1 = w0 * l2 + w1 * l3;
      if (!(l1 > 0.0)) continue;
      const V3 r1 = scl(y[0], l1), r2 = scl(y[1], l2), r3 = scl(y[2], l3);
      const V3 yd1 = sub(r1, r2), yd2 = sub(r1, r3), yn = cross(yd1, yd2);
      const double Y[9] = {yd1.x, yd2.x, yn.x, yd1.y, yd2.y, yn.y, yd1.z, yd2.z, yn.z};
      double* R = Rs[ns];
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[3 * i + j] = Y[3 * i] * Xi[j] + Y[3 * i + 1] * Xi[3 + j] + Y[3 * i + 2] * Xi[6 + j];
      ts[ns] = sub(r1, mulv(R, x[0]));
      ++ns;
    }
  }
  return ns;
}

// max |R R^T - I|: R = Y X^-1 is a rotation only when the three depths satisfy all three distance constraints
__device__ __forceinline__ double pnp_orth_err(const double* R) {
  double m = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double d = R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1] + R[3 * i + 2] * R[3 * j + 2] - (i == j ? 1.0 : 0.0);
      m = fmax(m, fabs(d));
    }
  return m;
}

__device__ __forceinline__ void pnp_load_k(const float* K, int b, double* Kd) {
  for (int i = 0; i < 9; ++i) Kd[i] = (double)K[9 * b + i];
}

// ---- hypotheses ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void pnp_hyp_kernel(const float* __restrict__ corr, const int32_t* __restrict__ count,
                                                     const float* __restrict__ Kin, int N, int n_hyp, uint32_t seed,
                                                     float* __restrict__ hyp_M, double* __restrict__ hyp_pose, int32_t* __restrict__ hyp_ok) {
  const int b = blockIdx.y, h = blockIdx.x * 64 + threadIdx.x;
  if (h >= n_hyp) return;
  const int64_t hi = (int64_t)b * n_hyp + h;
  const int cnt = count[b];
  float M[12] = {};
  double P[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  int ok = 0;
  int idx[4];
  int got = 0;
  if (cnt >= 4) {
    for (uint32_t c = 0; c < PNP_MAX_DRAWS && got < 4; ++c) {
      const int i = (int)(pnp_hash(seed, (uint32_t)b, (uint32_t)h, c) % (uint32_t)cnt);
      bool dup = false;
      for (int k = 0; k < got; ++k) dup |= idx[k] == i;
      if (!dup) idx[got++] = i;
    }
  }
  if (got == 4) {
    double K[9], Ki[9];
    pnp_load_k(Kin, b, K);
    adj3(K, Ki);
    const double dk = det3(K);
    for (int i = 0; i < 9; ++i) Ki[i] /= dk;
    const float* cb = corr + (int64_t)b * 5 * N;
    V3 x[4], y[4];
    double u[4], v[4];
    for (int k = 0; k < 4; ++k) {
      x[k] = v3(cb[idx[k]], cb[N + idx[k]], cb[2 * N + idx[k]]);
      u[k] = cb[3 * N + idx[k]];
      v[k] = cb[4 * N + idx[k]];
      const V3 r = mulv(Ki, v3(u[k], v[k], 1.0));
      y[k] = scl(r, 1.0 / sqrt(dot(r, r)));
    }
    double Rs[4][9];
    V3 ts[4];
    const int ns = pnp_p3p(x, y, Rs, ts);
    double beste = 0.0;
    int pick = -1;
    for (int k = 0; k < ns; ++k) {
      const V3 pc = v3(dot(v3(Rs[k][0], Rs[k][1], Rs[k][2]), x[3]) + ts[k].x, dot(v3(Rs[k][3], Rs[k][4], Rs[k][5]), x[3]) + ts[k].y,
                       dot(v3(Rs[k][6], Rs[k][7], Rs[k][8]), x[3]) + ts[k].z);
      const V3 p = mulv(K, pc);
      if (!(pc.z > 0.0)) continue;
      const double du = p.x / p.z - u[3], dv = p.y / p.z - v[3];
      const double e = du * du + dv * dv;
      if (!isfinite(e)) continue;
      bool fin = isfinite(ts[k].x) && isfinite(ts[k].y) && isfinite(ts[k].z);
      for (int i = 0; i < 9; ++i) fin = fin && isfinite(Rs[k][i]);
      if (!fin || !(pnp_orth_err(Rs[k]) <= PNP_ORTH_TOL)) continue;       // near-degenerate splits can give a non-rotation
      if (pick < 0 || e < beste) { beste = e; pick = k; }
    }
    if (pick >= 0) {
      const double tp[3] = {ts[pick].x, ts[pick].y, ts[pick].z};
      cmr_pnp_kmat(K, Rs[pick], tp, M);
      bool fin = true;
      for (int i = 0; i < 12; ++i) fin = fin && isfinite(M[i]);
      if (fin) {
        ok = 1;
        for (int i = 0; i < 9; ++i) P[i] = Rs[pick][i];
        P[9] = ts[pick].x; P[10] = ts[pick].y; P[11] = ts[pick].z;
      } else {
        for (int i = 0; i < 12; ++i) M[i] = 0.f;
      }
    }
  }
  for (int i = 0; i < 12; ++i) hyp_M[hi * 12 + i] = M[i];
  for (int i = 0; i < 12; ++i) hyp_pose[hi * 12 + i] = P[i];
  hyp_ok[hi] = ok;
}

// ---- scoring -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PNP_HYP_WG) void pnp_score_kernel(const float* __restrict__ corr, const int32_t* __restrict__ count,
                                                               const float* __restrict__ hyp_M, int N, int n_hyp, float thr2,
                                                               int32_t* __restrict__ hyp_cnt) {
  __shared__ float4 sp[PNP_SLICE];          // X, Y, Z, u
  __shared__ float sv[PNP_SLICE];           // v
  const int b = blockIdx.z;
  const int c0 = blockIdx.y * PNP_SLICE;
  const int cnt = count[b];
  if (c0 >= cnt) return;                    // block-uniform
  const int nloc = min(PNP_SLICE, cnt - c0);
  const float* cb = corr + (int64_t)b * 5 * N + c0;
  for (int i = threadIdx.x; i < nloc; i += PNP_HYP_WG) {
    sp[i] = make_float4(cb[i], cb[N + i], cb[2 * N + i], cb[3 * N + i]);
    sv[i] = cb[4 * N + i];
  }
  const int h = blockIdx.x * PNP_HYP_WG + threadIdx.x;
  float M[12];
  const bool hv = h < n_hyp;
  const float* src = hyp_M + ((int64_t)b * n_hyp + (hv ? h : 0)) * 12;
#pragma unroll
  for (int i = 0; i < 12; ++i) M[i] = hv ? src[i] : 0.f;
  __syncthreads();
  int n = 0;
#pragma unroll 4
  for (int i = 0; i < nloc; ++i) {
    const float4 p = sp[i];
    n += cmr_pnp_inlier(M, p.x, p.y, p.z, p.w, sv[i], thr2) ? 1 : 0;
  }
  if (hv && n) atomicAdd(&hyp_cnt[(int64_t)b * n_hyp + h], n);
}

// ---- selection + Gauss-Newton + recount ----------------------------------------------------------------------------------------
__device__ __forceinline__ int pnp_block_count(int v, int* scratch) {      // sum over the block (integers: order free); all threads
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if (lane == 0) scratch[wave] = v;
  __syncthreads();
  int s = 0;
  for (int w = 0; w < PNP_SEL_THREADS / 64; ++w) s += scratch[w];
  return s;
}

__global__ __launch_bounds__(PNP_SEL_THREADS) void pnp_select_kernel(const float* __restrict__ corr, const int32_t* __restrict__ count,
                                                                     const float* __restrict__ Kin, int N, int n_hyp, float thr2,
                                                                     int refine_iters, const float* __restrict__ hyp_M,
                                                                     const double* __restrict__ hyp_pose,
                                                                     const int32_t* __restrict__ hyp_ok, const int32_t* __restrict__ hyp_cnt,
                                                                     float* __restrict__ pose, int32_t* __restrict__ inliers,
                                                                     int32_t* __restrict__ status, int32_t* __restrict__ hyp_inliers) {
  __shared__ long long key[PNP_SEL_THREADS];
  __shared__ double acc[PNP_SEL_THREADS / 64][PNP_NACC];
  __shared__ int scratch[PNP_SEL_THREADS / 64];
  __shared__ double sh_pose[12];            // the pose every thread evaluates (R row-major, t)
  __shared__ int sh_stop;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cnt = count[b];
  // most inliers, ties to the lowest hypothesis index; invalid hypotheses count -1
  long long k = -1;
  for (int h = tid; h < n_hyp; h += PNP_SEL_THREADS) {
    const int64_t hi = (int64_t)b * n_hyp + h;
    const int c = hyp_ok[hi] ? hyp_cnt[hi] : -1;
    if (hyp_inliers) hyp_inliers[hi] = c;
    const long long kk = ((long long)(c + 1) << 32) | (long long)(0x7fffffff - h);
    if (kk > k) k = kk;
  }
  key[tid] = k;
  __syncthreads();
  for (int s = PNP_SEL_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s && key[tid + s] > key[tid]) key[tid] = key[tid + s];
    __syncthreads();
  }
  const long long best = key[0];
  const int bc = (int)(best >> 32) - 1;
  const int bh = 0x7fffffff - (int)(best & 0xffffffffll);
  float* out = pose + 16 * b;
  if (cnt < 4 || bc < 0) {
    if (tid < 16) out[tid] = (tid % 5 == 0) ? 1.f : 0.f;
    if (tid == 0) { inliers[b] = 0; status[b] = cnt < 4 ? 1 : 2; }
    return;
  }
  const int64_t bhi = (int64_t)b * n_hyp + bh;
  float Mh[12];
  for (int i = 0; i < 12; ++i) Mh[i] = hyp_M[bhi * 12 + i];
  double K[9];
  pnp_load_k(Kin, b, K);
  const float* cb = corr + (int64_t)b * 5 * N;
  if (tid < 12) sh_pose[tid] = hyp_pose[bhi * 12 + tid];
  if (tid == 0) sh_stop = 0;
  __syncthreads();
  double prev[12], cost_prev = 0.0;
  for (int it = 0; refine_iters > 0 && it <= refine_iters; ++it) {
    double R[9], t[3];
    for (int i = 0; i < 9; ++i) R[i] = sh_pose[i];
    for (int i = 0; i < 3; ++i) t[i] = sh_pose[9 + i];
    double a[PNP_NACC] = {};
    for (int i = tid; i < cnt; i += PNP_SEL_THREADS) {
      const float X = cb[i], Y = cb[N + i], Z = cb[2 * N + i], u = cb[3 * N + i], v = cb[4 * N + i];
      if (!cmr_pnp_inlier(Mh, X, Y, Z, u, v, thr2)) continue;
      cmr_pnp_terms(K, R, t, X, Y, Z, u, v, a);
    }
    for (int q = 0; q < PNP_NACC; ++q) {
      const double s = cmr_wave_sum_d(a[q]);
      if (lane == 0) acc[wave][q] = s;
    }
    __syncthreads();
    if (tid == 0) {
      double tot[PNP_NACC];
      for (int q = 0; q < PNP_NACC; ++q) {
        double s = 0.0;
        for (int w = 0; w < PNP_SEL_THREADS / 64; ++w) s += acc[w][q];
        tot[q] = s;
      }
      const double cost = tot[27];
      int stop = 0;
      if (it > 0 && !(cost < cost_prev)) {
        for (int i = 0; i < 12; ++i) sh_pose[i] = prev[i];                 // the step did not lower the cost: undo it
        stop = 1;
      } else if (it == refine_iters) {
        stop = 1;
      } else {
        double g[6], dx[6];
        for (int r = 0; r < 6; ++r) g[r] = -tot[21 + r];
        if (!cmr_pnp_chol6<false>(tot, g, dx)) {
          stop = 1;
        } else {
          for (int i = 0; i < 12; ++i) prev[i] = sh_pose[i];
          cost_prev = cost;
          double nw[12];
          cmr_pose_left_update(prev, dx, nw);              // a pose that is not finite fails the next pass' cost test and is undone there
          for (int i = 0; i < 12; ++i) sh_pose[i] = nw[i];
        }
      }
      sh_stop = stop;
    }
    __syncthreads();
    if (sh_stop) break;
    __syncthreads();                                       // acc is rewritten by the next pass
  }
  // recount with the refined pose; keep it if it has at least the hypothesis' inliers
  float Mr[12];
  double Rf[9];
  for (int i = 0; i < 9; ++i) Rf[i] = sh_pose[i];
  const double tf[3] = {sh_pose[9], sh_pose[10], sh_pose[11]};
  cmr_pnp_kmat(K, Rf, tf, Mr);
  int n = 0;
  if (refine_iters > 0)
    for (int i = tid; i < cnt; i += PNP_SEL_THREADS) n += cmr_pnp_inlier(Mr, cb[i], cb[N + i], cb[2 * N + i], cb[3 * N + i], cb[4 * N + i], thr2);
  const int rc = refine_iters > 0 ? pnp_block_count(n, scratch) : -1;
  const bool use_ref = refine_iters > 0 && rc >= bc;
  if (tid < 16) out[tid] = use_ref ? cmr_pose_entry(sh_pose, tid) : cmr_pose_entry(hyp_pose + bhi * 12, tid);
  if (tid == 0) { inliers[b] = use_ref ? rc : bc; status[b] = 0; }
}

struct PnpWs {
  size_t pose, M, ok, cnt, chunk, count, corr, total;
};

static size_t pnp_align(size_t v) { return (v + 255) & ~(size_t)255; }

static PnpWs pnp_layout(int B, int N, int n_hyp) {
  PnpWs w;
  const size_t H = (size_t)B * n_hyp;
  const int nchunk = (N + PNP_CHUNK - 1) / PNP_CHUNK;
  w.pose = 0;
  w.M = pnp_align(w.pose + H * 12 * sizeof(double));
  w.ok = pnp_align(w.M + H * 12 * sizeof(float));
  w.cnt = pnp_align(w.ok + H * sizeof(int32_t));
  w.chunk = pnp_align(w.cnt + H * sizeof(int32_t));
  w.count = pnp_align(w.chunk + (size_t)B * nchunk * sizeof(int32_t));
  w.corr = pnp_align(w.count + (size_t)B * sizeof(int32_t));
  w.total = pnp_align(w.corr + (size_t)B * 5 * N * sizeof(float));
  return w;
}

}  // namespace

extern "C" int64_t cmr_pnp_ransac_workspace_bytes(int B, int N, int n_hyp) {
  if (B <= 0 || N <= 0 || n_hyp <= 0) return 0;
  return (int64_t)pnp_layout(B, N, n_hyp).total;
}

extern "C" int cmr_pnp_ransac_f32(const float* pts, const float* uv, const void* mask, int mask_bytes, const float* K, int B, int N,
                                  int n_hyp, float thr, uint32_t seed, int refine_iters, float* pose, int32_t* inliers, int32_t* status,
                                  int32_t* hyp_inliers, void* ws, int64_t ws_bytes, hipStream_t stream) {
  CMR_REQUIRE(pts && uv && mask && K && pose && inliers && status && ws);
  CMR_REQUIRE(B > 0 && B <= 65535 && N > 0 && N <= 65535 * PNP_SLICE && n_hyp > 0 && n_hyp <= (1 << 20) && refine_iters >= 0);
  CMR_REQUIRE(mask_bytes == 1 || mask_bytes == 8);
  CMR_REQUIRE(thr > 0.f && __builtin_isfinite(thr));
  CMR_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7u) == 0);
  CMR_REQUIRE(ws_bytes >= cmr_pnp_ransac_workspace_bytes(B, N, n_hyp));
  const PnpWs w = pnp_layout(B, N, n_hyp);
  char* base = (char*)ws;
  double* hyp_pose = (double*)(base + w.pose);
  float* hyp_M = (float*)(base + w.M);
  int32_t* hyp_ok = (int32_t*)(base + w.ok);
  int32_t* hyp_cnt = (int32_t*)(base + w.cnt);
  int32_t* chunk_cnt = (int32_t*)(base + w.chunk);
  int32_t* count = (int32_t*)(base + w.count);
  float* corr = (float*)(base + w.corr);
  const int nchunk = (N + PNP_CHUNK - 1) / PNP_CHUNK;
  const int nslice = (N + PNP_SLICE - 1) / PNP_SLICE;
  const float thr2 = thr * thr;
  if (hipMemsetAsync(hyp_cnt, 0, (size_t)B * n_hyp * sizeof(int32_t), stream) != hipSuccess) return CMR_ELAUNCH;
  hipLaunchKernelGGL(pnp_chunk_count_kernel, dim3(nchunk, B), dim3(PNP_CHUNK), 0, stream, mask, mask_bytes, N, nchunk, chunk_cnt);
  hipLaunchKernelGGL(pnp_pack_kernel, dim3(nchunk, B), dim3(PNP_CHUNK), 0, stream, pts, uv, mask, mask_bytes, N, nchunk,
                     (const int32_t*)chunk_cnt, corr, count);
  hipLaunchKernelGGL(pnp_hyp_kernel, dim3((n_hyp + 63) / 64, B), dim3(64), 0, stream, (const float*)corr, (const int32_t*)count, K, N,
                     n_hyp, seed, hyp_M, hyp_pose, hyp_ok);
  hipLaunchKernelGGL(pnp_score_kernel, dim3((n_hyp + PNP_HYP_WG - 1) / PNP_HYP_WG, nslice, B), dim3(PNP_HYP_WG), 0, stream,
                     (const float*)corr, (const int32_t*)count, (const float*)hyp_M, N, n_hyp, thr2, hyp_cnt);
  hipLaunchKernelGGL(pnp_select_kernel, dim3(B), dim3(PNP_SEL_THREADS), 0, stream, (const float*)corr, (const int32_t*)count, K, N, n_hyp,
                     thr2, refine_iters, (const float*)hyp_M, (const double*)hyp_pose, (const int32_t*)hyp_ok, (const int32_t*)hyp_cnt,
                     pose, inliers, status, hyp_inliers);
  return cmr_launch_status();
}
