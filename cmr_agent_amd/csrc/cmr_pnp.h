// The pieces that PnP-RANSAC (pnp.hip) and the refinement from a given pose (pnp_refine.hip) must agree
// on, stated once: the working set of the refinement IS RANSAC's inlier set, and its step is RANSAC's Gauss-Newton step.  Device code
// only.
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
