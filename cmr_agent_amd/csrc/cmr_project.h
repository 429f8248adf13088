// Projection of a cloud row through a pose, stated once for every operation that does it: guided match,
// pose score, visibility, paint and render.  Their contract is that "in view", the cell and uv agree BIT FOR BIT between them, so none
// of them keeps a chain or a predicate of its own.  Device code only.
#pragma once
#include "cmr_common.h"

// The limits the pose operations share, each defined here and nowhere else (ops.py restates them for its messages).
constexpr int CMR_MAX_RADIUS = 16;    // a window's radius in pixels: (2r + 1)^2 <= 1089 cells per row; also keeps centre +- r far from integer overflow
constexpr int CMR_MAX_PLANES = 64;    // planes of an image that is sampled or of an attribute that is rendered
constexpr int CMR_MAX_POSES = 4096;   // candidate poses per sample

// X_c = R x + t, p = K X_c in fp32.  P is the sample's 4 x 4 pose, row-major (16 floats, the last row unused), K its 3 x 3 intrinsics
// (9 floats), x its cloud as three planes of N.  Every sum is an fmaf chain from the LAST term inwards; K[2] zc, K[5] zc and K[8] zc are
// plain products.  A restatement elsewhere (the tests' fp32 torch code) must use these operations in this order.
__device__ __forceinline__ void cmr_project_chains(const float* P, const float* K, float X, float Y, float Z,
                                                   float& p0, float& p1, float& p2) {
  const float xc = fmaf(P[0], X, fmaf(P[1], Y, fmaf(P[2], Z, P[3])));
  const float yc = fmaf(P[4], X, fmaf(P[5], Y, fmaf(P[6], Z, P[7])));
  const float zc = fmaf(P[8], X, fmaf(P[9], Y, fmaf(P[10], Z, P[11])));
  p0 = fmaf(K[0], xc, fmaf(K[1], yc, K[2] * zc));
  p1 = fmaf(K[3], xc, fmaf(K[4], yc, K[5] * zc));
  p2 = fmaf(K[6], xc, fmaf(K[7], yc, K[8] * zc));
}
__device__ __forceinline__ void cmr_project_chains(const float* P, const float* K, const float* x, int N, int n, float& p0, float& p1,
                                                   float& p2) {
  cmr_project_chains(P, K, x[n], x[N + n], x[2 * N + n], p0, p1, p2);
}

// X_c alone, by the same three chains (the same bits as inside cmr_project_chains), and a direction turned by R alone -- the pattern
// without the translation, the last term a plain product: for a caller that needs the camera-frame point and normal (surfel.hip).
__device__ __forceinline__ void cmr_camera_chains(const float* P, float X, float Y, float Z, float& xc, float& yc, float& zc) {
  xc = fmaf(P[0], X, fmaf(P[1], Y, fmaf(P[2], Z, P[3])));
  yc = fmaf(P[4], X, fmaf(P[5], Y, fmaf(P[6], Z, P[7])));
  zc = fmaf(P[8], X, fmaf(P[9], Y, fmaf(P[10], Z, P[11])));
}
__device__ __forceinline__ void cmr_rotate_chains(const float* P, float X, float Y, float Z, float& xc, float& yc, float& zc) {
  xc = fmaf(P[0], X, fmaf(P[1], Y, P[2] * Z));
  yc = fmaf(P[4], X, fmaf(P[5], Y, P[6] * Z));
  zc = fmaf(P[8], X, fmaf(P[9], Y, P[10] * Z));
}

struct CmrProj {
  float u, v, z;      // (u, v) = (p0 / p2, p1 / p2); z = p2, the depth
  bool view;
  int cx, cy;         // rintf of u and v (round half to even) where view, else 0
  int cell;           // cy * w + cx (< h * w <= 2^24) where view, else -1; cmr_project<true> only, which leaves cx and cy 0
};

// "In view", decided on the FLOATS: p2 > 0, u and v finite, and the (2r + 1)^2 window round the rounded centre touches the h x w map:
// cx + r >= 0, cx - r <= w - 1, cy + r >= 0, cy - r <= h - 1.  r = 0 is the test visibility, paint and render use: the centre is a cell.
// Two forms of the one predicate.  With branches: u, v and z are NaN where p2 <= 0 and nothing is divided there.  CELL chooses what the
// rounded centre is handed back as: the pair (cx, cy), or the cell number for a caller that stores it (visibility.hip) -- computed
// where the predicate is decided, because the compiler folds the conversions into a select there and nowhere else.
template <bool CELL = false>
__device__ __forceinline__ CmrProj cmr_project(const float* P, const float* K, const float* x, int N, int n, int h, int w, int radius) {
  CmrProj r;
  float p0, p1, p2;
  cmr_project_chains(P, K, x, N, n, p0, p1, p2);
  r.u = r.v = r.z = __builtin_nanf("");
  r.view = false;
  r.cx = 0;
  r.cy = 0;
  r.cell = -1;
  if (p2 > 0.f) {
    r.z = p2;
    r.u = p0 / p2;
    r.v = p1 / p2;
    if (isfinite(r.u) && isfinite(r.v)) {
      const float cx = rintf(r.u), cy = rintf(r.v), rf = (float)radius;
      r.view = cx + rf >= 0.f && cx - rf <= (float)(w - 1) && cy + rf >= 0.f && cy - rf <= (float)(h - 1);
      if (r.view) {
        if (CELL) {
          r.cell = (int)cy * w + (int)cx;
        } else {
          r.cx = (int)cx;
          r.cy = (int)cy;
        }
      }
    }
  }
  return r;
}

// Without branches, for a caller whose lanes must stay in step (pose_score.hip: DPP moves follow): u and v are divided whatever p2 is,
// the predicate is one run of compares joined by & (no short-circuit branches) and the centre is a select.  The same truth value and,
// where view, the same u, v, cx, cy as cmr_project.
__device__ __forceinline__ CmrProj cmr_project_select(const float* P, const float* K, float X, float Y, float Z, int h, int w, float rf) {
  CmrProj r;
  float p0, p1, p2;
  cmr_project_chains(P, K, X, Y, Z, p0, p1, p2);
  r.u = p0 / p2;
  r.v = p1 / p2;
  r.z = p2;
  r.cell = -1;        // not provided in this form
  const float cx = rintf(r.u), cy = rintf(r.v);
  r.view = (p2 > 0.f) & isfinite(r.u) & isfinite(r.v) & (cx + rf >= 0.f) & (cx - rf <= (float)(w - 1)) & (cy + rf >= 0.f) &
           (cy - rf <= (float)(h - 1));
  r.cx = (int)(r.view ? cx : 0.f);
  r.cy = (int)(r.view ? cy : 0.f);
  return r;
}
