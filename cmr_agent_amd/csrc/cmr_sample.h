// Sampling of a planar image at a projected point, stated once for the operations that do it: paint and pose MI.
// Their contract is that the value a row takes agrees BIT FOR BIT between them, so neither keeps taps or lerps of its own.  Device code only.
#pragma once
#include "cmr_project.h"

__device__ __forceinline__ int cmr_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// Tap offsets inside one H x W plane for a row IN VIEW at radius 0, all inside the plane.  Nearest: o00 = the cell (rint u, rint v), the
// rest unused.  Bilinear: pixel centres on the integers, x0 = floorf u, fx = u - x0 (likewise y), the four taps (x0, y0) .. (x0 + 1,
// y0 + 1) with every index clamped to the plane (border replicate).  A row that is not in view gets offset 0 everywhere: it may load,
// and its value is dropped.
struct CmrTaps {
  int o00, o01, o10, o11;
  float fx, fy;
};

template <bool BILINEAR>
__device__ __forceinline__ CmrTaps cmr_taps(const CmrProj& p, bool take, int H, int W) {
  CmrTaps t;
  t.o00 = t.o01 = t.o10 = t.o11 = 0;
  t.fx = t.fy = 0.f;
  if (take) {
    if (BILINEAR) {
      const float xf = floorf(p.u), yf = floorf(p.v);                    // in [-1, W - 1] / [-1, H - 1]: u >= -0.5 where in view
      t.fx = __fsub_rn(p.u, xf);
      t.fy = __fsub_rn(p.v, yf);
      const int x0 = (int)xf, y0 = (int)yf;
      const int xa = cmr_clampi(x0, W - 1), xb = cmr_clampi(x0 + 1, W - 1), ya = cmr_clampi(y0, H - 1), yb = cmr_clampi(y0 + 1, H - 1);
      t.o00 = ya * W + xa; t.o01 = ya * W + xb; t.o10 = yb * W + xa; t.o11 = yb * W + xb;
    } else {
      t.o00 = p.cy * W + p.cx;
    }
  }
  return t;
}

// The value from the loaded taps: the three lerps rounded operation by operation (cmr_lerp: never an fma).
template <bool BILINEAR>
__device__ __forceinline__ float cmr_tap_value(const CmrTaps& t, float i00, float i01, float i10, float i11) {
  return BILINEAR ? cmr_lerp(cmr_lerp(i00, i01, t.fx), cmr_lerp(i10, i11, t.fx), t.fy) : i00;
}
