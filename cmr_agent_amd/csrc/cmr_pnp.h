// The pieces that PnP-RANSAC (pnp.hip) and the refinement from a given pose (pnp_refine.hip) must agree
// on, stated once: the working set of the refinement IS RANSAC's inlier set, and its step is RANSAC's Gauss-Newton step.  The working
// pose of that step -- its load, left update, fp32 4x4 form and the slice-order sum of a step's slots -- serves point-to-plane ICP
// (cloud_icp.hip) as well.  Device code only.
#pragma once
#include "cmr_common.h"

// The draws of a RANSAC hypothesis (pnp.hip; cloud_global.hip with b = 0).
// lowbias32 (C. Wellons' integer hash, constants 0x21f0aaad / 0xd35a2d97); draw c of hypothesis h of sample b:
// mix(mix(mix(mix(seed ^ 0x9e3779b9) ^ b) ^ h) ^ c) % count.
__host__ __device__ __forceinline__ uint32_t pnp_mix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x21f0aaadu;
  x ^= x >> 15;
  x *= 0xd35a2d97u;
  x ^= x >> 15;
  return x;
}

__device__ __forceinline__ uint32_t pnp_hash(uint32_t seed, uint32_t b, uint32_t h, uint32_t c) {
  return pnp_mix(pnp_mix(pnp_mix(pnp_mix(seed ^ 0x9e3779b9u) ^ b) ^ h) ^ c);
}

// The inlier test (scoring, selection, recount and the refinement's working set: the same operations in the same order).
// M = K[R|t] row-major fp32; inlier iff z > 0 and (x - u z)^2 + (y - v z)^2 <= thr^2 z^2 (no division).
__device__ __forceinline__ bool cmr_pnp_inlier(const float* M, float X, float Y, float Z, float u, float v, float thr2) {
  const float x = fmaf(M[0], X, fmaf(M[1], Y, fmaf(M[2], Z, M[3])));
  const float y = fmaf(M[4], X, fmaf(M[5], Y, fmaf(M[6], Z, M[7])));
  const float z = fmaf(M[8], X, fmaf(M[9], Y, fmaf(M[10], Z, M[11])));
  const float ex = fmaf(-u, z, x), ey = fmaf(-v, z, y);
  const float e2 = fmaf(ex, ex, ey * ey);
  return z > 0.f && e2 <= thr2 * (z * z);
}

// K [R | t] -> fp32 row-major 3x4; every entry a float64 sum of three products, left to right, rounded once
__device__ __forceinline__ void cmr_pnp_kmat(const double* K, const double* R, const double* t, float* M) {
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) M[4 * i + j] = (float)(K[3 * i] * R[j] + K[3 * i + 1] * R[3 + j] + K[3 * i + 2] * R[6 + j]);
    M[4 * i + 3] = (float)(K[3 * i] * t[0] + K[3 * i + 1] * t[1] + K[3 * i + 2] * t[2]);
  }
}

// Rodrigues: exp([w]x)
static __device__ void cmr_pnp_expso3(const double* w, double* E) {
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  const double th = sqrt(th2);
  double a, c;
  if (th < 1e-8) { a = 1.0 - th2 / 6.0; c = 0.5 - th2 / 24.0; }
  else { a = sin(th) / th; c = (1.0 - cos(th)) / th2; }
  const double W[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double ww = 0.0;
      for (int k = 0; k < 3; ++k) ww += W[3 * i + k] * W[3 * k + j];
      E[3 * i + j] = (i == j ? 1.0 : 0.0) + a * W[3 * i + j] + c * ww;
    }
}

// ---- the working pose of a Gauss-Newton loop: 12 doubles, R row-major then t (pnp.hip, pnp_refine.hip, cloud_icp.hip) ----------------
// What a loop does with a step -- PnP's accept / undo, ICP's stop and status -- differs on purpose and stays in its kernel.
constexpr int CMR_GN_NACC = 28;      // the sums of a step: J^T J (21 upper-triangle entries, row by row), J^T r (6), cost

// from a row-major fp32 4x4
__device__ __forceinline__ void cmr_pose_load(const float* P, double* cur) {
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) cur[3 * i + j] = (double)P[4 * i + j];
    cur[9 + i] = (double)P[4 * i + 3];
  }
}
// the left update nw = [Exp(w) | v] cur with xi = (w, v); -> whether every entry of nw is finite (nw is written either way).  The three
// arrays do not overlap, and say so: without it prf_step_kernel took 76 VGPRs instead of 72 and lost a wave per SIMD.
__device__ __forceinline__ bool cmr_pose_left_update(const double* __restrict__ cur, const double* __restrict__ xi,
                                                     double* __restrict__ nw) {
  double E[9];
  cmr_pnp_expso3(xi, E);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) nw[3 * i + j] = E[3 * i] * cur[j] + E[3 * i + 1] * cur[3 + j] + E[3 * i + 2] * cur[6 + j];
    nw[9 + i] = E[3 * i] * cur[9] + E[3 * i + 1] * cur[10] + E[3 * i + 2] * cur[11] + xi[3 + i];
  }
  bool ok = true;
  for (int i = 0; i < 12; ++i) ok = ok && isfinite(nw[i]);
  return ok;
}
// element e < 16 of the pose as a row-major fp32 4x4: threads 0..15 write one each
__device__ __forceinline__ float cmr_pose_entry(const double* cur, int e) {
  const int r = e >> 2, c = e & 3;
  return r == 3 ? (c == 3 ? 1.f : 0.f) : (float)(c < 3 ? cur[3 * r + c] : cur[9 + r]);
}
// entry `q` of the step's sums: the slices' slots added IN SLICE ORDER; eight loads in flight, added in that same order
__device__ __forceinline__ double cmr_slot_sum(const double* __restrict__ slots, int nslice, int q) {
  double v = 0.0;
  int s = 0;
  for (; s + 8 <= nslice; s += 8) {
    double t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = slots[(int64_t)(s + u) * CMR_GN_NACC + q];
#pragma unroll
    for (int u = 0; u < 8; ++u) v += t[u];
  }
  for (; s < nslice; ++s) v += slots[(int64_t)s * CMR_GN_NACC + q];
  return v;
}

// One correspondence's reprojection terms under the pose (R, t) and the intrinsics K (row-major 3x3), added into a: J^T J (upper triangle),
// J^T r and the cost, for the residual (pu - u, pv - v) and a left increment of the pose.  false, and nothing added, for a point that does
// not project in front of the camera (p2 <= 0, or not a number).
__device__ __forceinline__ bool cmr_pnp_terms(const double* K, const double* R, const double* t, float X, float Y, float Z, float u, float v,
                                              double (&a)[CMR_GN_NACC]) {
  const double xc0 = R[0] * X + R[1] * Y + R[2] * Z + t[0], xc1 = R[3] * X + R[4] * Y + R[5] * Z + t[1],
               xc2 = R[6] * X + R[7] * Y + R[8] * Z + t[2];
  const double p0 = K[0] * xc0 + K[1] * xc1 + K[2] * xc2, p1 = K[3] * xc0 + K[4] * xc1 + K[5] * xc2,
               p2 = K[6] * xc0 + K[7] * xc1 + K[8] * xc2;
  if (!(p2 > 0.0)) return false;
  const double iz = 1.0 / p2, pu = p0 * iz, pv = p1 * iz;
  const double ru = pu - u, rv = pv - v;
  const double ga[3] = {(K[0] - K[6] * pu) * iz, (K[1] - K[7] * pu) * iz, (K[2] - K[8] * pu) * iz};     // d pu / d xc
  const double gb[3] = {(K[3] - K[6] * pv) * iz, (K[4] - K[7] * pv) * iz, (K[5] - K[8] * pv) * iz};
  // d / d omega (left increment): xc x g
  const double ja[6] = {xc1 * ga[2] - xc2 * ga[1], xc2 * ga[0] - xc0 * ga[2], xc0 * ga[1] - xc1 * ga[0], ga[0], ga[1], ga[2]};
  const double jb[6] = {xc1 * gb[2] - xc2 * gb[1], xc2 * gb[0] - xc0 * gb[2], xc0 * gb[1] - xc1 * gb[0], gb[0], gb[1], gb[2]};
  int q = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int cc = r; cc < 6; ++cc) a[q++] += ja[r] * ja[cc] + jb[r] * jb[cc];
#pragma unroll
  for (int r = 0; r < 6; ++r) a[21 + r] += ja[r] * ru + jb[r] * rv;
  a[27] += ru * ru + rv * rv;
  return true;
}

// Cholesky solve of the 6x6 H x = g (H from the 21 upper-triangle entries, row by row); false if H is not positive definite.  With
// REL_PIVOT a pivot must also exceed CMR_PNP_PIVOT_TOL times its diagonal entry: a rank-deficient H (all rows on a line) leaves a pivot
// of rounding noise, ~1e-16 of the diagonal with either sign, and the refinement's "status 2" must not hang on that sign.  RANSAC's own
// step keeps the plain test it was released with; the arithmetic is the same for both.
constexpr double CMR_PNP_PIVOT_TOL = 1e-13;
template <bool REL_PIVOT>
static __device__ bool cmr_pnp_chol6(const double* Hu, const double* g, double* x) {
  double L[36] = {};
  double H[36];
  int k = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) { H[6 * i + j] = Hu[k]; H[6 * j + i] = Hu[k]; ++k; }
  for (int j = 0; j < 6; ++j) {
    double d = H[6 * j + j];
    for (int p = 0; p < j; ++p) d -= L[6 * j + p] * L[6 * j + p];
    if (!(d > 0.0 && (!REL_PIVOT || d > CMR_PNP_PIVOT_TOL * H[6 * j + j]))) return false;
    L[6 * j + j] = sqrt(d);
    for (int i = j + 1; i < 6; ++i) {
      double s = H[6 * i + j];
      for (int p = 0; p < j; ++p) s -= L[6 * i + p] * L[6 * j + p];
      L[6 * i + j] = s / L[6 * j + j];
    }
  }
  double z[6];
  for (int i = 0; i < 6; ++i) {
    double s = g[i];
    for (int p = 0; p < i; ++p) s -= L[6 * i + p] * z[p];
    z[i] = s / L[6 * i + i];
  }
  for (int i = 5; i >= 0; --i) {
    double s = z[i];
    for (int p = i + 1; p < 6; ++p) s -= L[6 * p + i] * x[p];
    x[i] = s / L[6 * i + i];
  }
  return true;
}
