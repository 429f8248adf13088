// The z-buffer, stated once: render_points and render_surfels share the owner z-buffer (key, fill, decode, attribute gather),
// visibility and depth_test the depth test of a row.  Their contracts are exact -- the renderers give the same index_map and depth_map bits
// for the same winners, depth_test on visibility's own map gives that call's flags -- so none keeps a key, a decode or a window walk of its own.
#pragma once
#include "cmr_sample.h"

// ---- the owner z-buffer: one 64-bit key per cell ------------------------------------------------------------------------------------
// (bits of depth) << 32 | row.  Positive floats order like their bits, so ONE unsigned 64-bit atomic min leaves the nearest row in the
// cell and the lowest row on equal depths, whatever the order of arrival.  All ones = no row (no depth has those bits: it is a NaN).
constexpr unsigned long long CMR_ZEMPTY = ~0ull;
constexpr int CMR_ZPLANES = 4;     // attribute planes whose gathers are in flight together

__device__ __forceinline__ unsigned long long cmr_zkey(float depth, unsigned row) {
  return ((unsigned long long)__builtin_bit_cast(unsigned, depth) << 32) | row;
}
__device__ __forceinline__ int cmr_zowner(unsigned long long key) { return (int)(unsigned)(key & 0xffffffffull); }
__device__ __forceinline__ float cmr_zdepth(unsigned long long key) { return __builtin_bit_cast(float, (unsigned)(key >> 32)); }

// key map = empty with 16-byte stores (the workspace is 16-byte aligned); i = the thread's index in the grid, stride = the grid's threads
__device__ __forceinline__ void cmr_zfill(unsigned long long* __restrict__ keys, int64_t cells, int64_t i, int64_t stride) {
  const int64_t nvec = cells >> 1;
  ulonglong2* kv = reinterpret_cast<ulonglong2*>(keys);
  for (int64_t v = i; v < nvec; v += stride) kv[v] = make_ulonglong2(CMR_ZEMPTY, CMR_ZEMPTY);
  if (i == 0 && (cells & 1)) keys[cells - 1] = CMR_ZEMPTY;
}

// The resolve tail of pixel i of sample b (valid: i < cells), one thread per pixel, in two halves so that a caller can put maps of its own
// between them.  First the index_map / depth_map stores from the winning key, -1 / +inf where no row owns the pixel; returns `owned`,
// under which cmr_zowner(best) is the row ...
__device__ __forceinline__ bool cmr_zresolve(unsigned long long best, bool valid, int b, int i, int cells, int32_t* index_map,
                                             float* depth_map) {
  const bool owned = valid && best != CMR_ZEMPTY;
  if (valid) {
    const int64_t o = (int64_t)b * cells + i;
    index_map[o] = owned ? cmr_zowner(best) : -1;
    depth_map[o] = owned ? cmr_zdepth(best) : __builtin_huge_valf();
  }
  return owned;
}
// ... then attr_map[b, c, i] = attr[b, c, owner], `fill` where not owned: coalesced stores, and the only scattered read, CMR_ZPLANES planes
// at a time with the plane index clamped (a plane past C loads plane C - 1 and stores nothing).
__device__ __forceinline__ void cmr_zgather(unsigned long long best, bool owned, bool valid, int b, int i, int cells,
                                            const float* attr, int C, int N, float fill, float* attr_map) {
  if (attr_map) {
    const float* ab = attr + (int64_t)b * C * N;
    float* ob = attr_map + (int64_t)b * C * cells;
    for (int c = 0; c < C; c += CMR_ZPLANES) {                             // wave-uniform
      float val[CMR_ZPLANES];
#pragma unroll
      for (int k = 0; k < CMR_ZPLANES; ++k) val[k] = fill;
      if (owned) {
#pragma unroll
        for (int k = 0; k < CMR_ZPLANES; ++k) val[k] = ab[(int64_t)(c + k < C ? c + k : C - 1) * N + cmr_zowner(best)];
      }
      if (valid) {
#pragma unroll
        for (int k = 0; k < CMR_ZPLANES; ++k)
          if (c + k < C) ob[(int64_t)(c + k) * cells + i] = val[k];
      }
    }
  }
}

// ---- the depth test of one row against a depth map Z [B, h, w] -----------------------------------------------------------------------
// CMR_ZT_LANES = 4 lanes (one DPP quad) per row, THREADS / 4 rows per workgroup.  From the row's cell c (or -1: not selected or not in
// view) and its depth z: zmin = the least Z over the (2r + 1)^2 window round the cell, walked directly, a line at a time, lane j taking
// the columns cx - r + j, + 4, ...; the window is one run of (2r + 1) lines x nch steps of 4 columns, CMR_ZT_AHEAD steps per turn with
// their loads in flight together.  Every loop bound is wave-uniform (all rows walk the whole square; a cell outside the map or past the
// line's end is read from the clamped address and replaced by +inf), so EXEC is full under the two quad-permute DPP moves in which the
// four partial minima meet; a wave without one active row skips the walk.  visible iff z <= bound = zmin * opr + abs_tol, the product
// and the sum rounded separately.  visible[g] is stored by lane 0 of the row; counts[STRIDE * b + 0..2] = (selected, active, visible)
// by one atomic per workgroup and word.
// NaN: fminf drops a NaN cell -- it counts as empty, as +inf does.  ops.visibility's own map never holds one (+inf or a positive
// depth); a map the caller brings (cmr_depth_test_f32) may.
constexpr int CMR_ZT_LANES = 4;
constexpr int CMR_ZT_AHEAD = 4;

template <int THREADS, int STRIDE>
__device__ __forceinline__ void cmr_ztest_row(const float* __restrict__ Z, int b, int h, int w, int radius, float opr, float abs_tol,
                                              bool valid, bool sel, int c, float z, int64_t g, uint8_t* __restrict__ visible,
                                              int32_t* __restrict__ counts) {
  __shared__ int part[3][THREADS / 64];
  const int j = threadIdx.x & (CMR_ZT_LANES - 1);
  const bool active = c >= 0;                                            // selected and in view
  const int cx = active ? c % w : 0, cy = active ? c / w : 0;
  const float* Zb = Z + (int64_t)b * h * w;
  const float inf = __builtin_huge_valf();
  float zmin = inf;
  if (__ballot(active)) {                                                // wave-uniform: EXEC stays full inside
    const int nch = (2 * radius + 1 + CMR_ZT_LANES - 1) / CMR_ZT_LANES, total = (2 * radius + 1) * nch;
    int dy = -radius, ch = 0;                                            // wave-uniform
    for (int k = 0; k < total; k += CMR_ZT_AHEAD) {
      float f[CMR_ZT_AHEAD];
      bool in[CMR_ZT_AHEAD];
#pragma unroll
      for (int u = 0; u < CMR_ZT_AHEAD; ++u) {
        const int dx = -radius + ch * CMR_ZT_LANES + j;
        const int x = cx + dx, y = cy + dy;                              // past the end of the run dy = r + 1: dropped by k + u < total
        in[u] = k + u < total && dx <= radius && x >= 0 && x < w && y >= 0 && y < h;
        f[u] = Zb[cmr_clampi(y, h - 1) * w + cmr_clampi(x, w - 1)];
        if (++ch == nch) { ch = 0; ++dy; }
      }
#pragma unroll
      for (int u = 0; u < CMR_ZT_AHEAD; ++u) zmin = fminf(zmin, in[u] ? f[u] : inf);
    }
  }
  zmin = fminf(zmin, cmr_fdpp<0xB1>(zmin));                               // quad_perm:[1,0,3,2]; outside every branch
  zmin = fminf(zmin, cmr_fdpp<0x4E>(zmin));                               // quad_perm:[2,3,0,1]
  const float bound = cmr_mul_add_rn(zmin, opr, abs_tol);                // two roundings, never one fma
  const bool vis = active && z <= bound;
  const bool first = j == 0;
  if (valid && first) visible[g] = vis ? 1 : 0;
  const bool flag[3] = {sel && first, active && first, vis && first};
  int cnt[3];
  cmr_block_counts<3, THREADS>(flag, part, cnt);
  if (threadIdx.x < 3 && cnt[threadIdx.x]) atomicAdd(&counts[STRIDE * b + threadIdx.x], cnt[threadIdx.x]);
}

// ---- host pieces shared by the entries ------------------------------------------------------------------------------------------------
// bytes of the key map of B h x w maps (0 for sizes no entry accepts); a row mask of bytes or of 64-bit words; attr and attr_map together
// with 1 .. CMR_MAX_PLANES planes, or neither and C = 0; the depth test's tolerances finite and >= 0, and 1 + rel_tol summed in double and
// rounded once; a depth map is read and written as floats
static inline int64_t cmr_zkeys_bytes(int B, int h, int w) { return B <= 0 || h <= 0 || w <= 0 ? 0 : cmr_up16((int64_t)B * h * w * 8); }
static inline bool cmr_mask_bytes_ok(int mask_bytes) { return mask_bytes == 1 || mask_bytes == 8; }
static inline bool cmr_attr_ok(const float* attr, const float* attr_map, int C) {
  return (attr == nullptr) == (attr_map == nullptr) && (attr ? (C >= 1 && C <= CMR_MAX_PLANES) : C == 0);
}
static inline bool cmr_tols_ok(float rel_tol, float abs_tol) {
  return rel_tol >= 0.f && abs_tol >= 0.f && __builtin_isfinite(rel_tol) && __builtin_isfinite(abs_tol);
}
static inline float cmr_one_plus(float rel_tol) { return (float)(1.0 + (double)rel_tol); }
static inline bool cmr_aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
