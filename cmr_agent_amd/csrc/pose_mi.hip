// Pose scoring by mutual information (port extension): for P candidate poses per sample, the joint histogram of a per-point
// attribute (the LiDAR reflectance) and the grey value of the pixel the point lands on, and from it the entropies and the mutual
// information -- the targetless camera-LiDAR criterion of Pandey et al.  A second witness beside pose_score.hip: it reads the sensors,
// not the geometric model's features.  Projection and "in view" are cmr_project.h's, the grey value is cmr_sample.h's, so the rows and
// values are cmr_paint_points_f32's at C = 1 bit for bit.
//
// Three launches on the caller's stream, no host round trip:
//   pmi_fill_kernel   hist, counts and selected = 0 (16-byte stores: hist is 16-byte aligned).
//   pmi_hist_kernel   grid (row slices x pose chunks x B, the sample fastest): a workgroup owns PMI_SLICE consecutive rows of one sample
//                     and `chunk` consecutive poses, chunk sized from nb so that the chunk's histograms (nb^2 x 4 B each) take at most
//                     PMI_LDS_BYTES of LDS.  A thread keeps its PMI_ROWS rows (n = slice start + k * 256 + tid: coalesced) in registers
//                     across the poses: x, y, z and a code = the attribute's bin, or -1 (selected, attribute not finite: can be in view,
//                     never counted) or -2 (not selected).  Per pose (workgroup-uniform: R, t and K arrive through scalar loads) the rows
//                     go PMI_AHEAD at a time: projection (the form without branches), tap offsets (0 for a row that takes nothing: it
//                     loads pixel 0 and a select drops it), all loads, then the grey bin and ONE LDS integer atomic per counted row.
//                     In-view rows are counted per thread, summed over the wave and added to an LDS word per pose.  At the end the
//                     workgroup adds its NON-ZERO bins to hist with global integer atomics -- plain stores when there is one slice, the
//                     fill covers the zeros -- and its in-view counts likewise; the chunk-0 workgroups add the slice's selected rows.
//   pmi_final_kernel  one workgroup per (b, p): the histogram into LDS, the marginals as integer sums, n = their total, then the three
//                     sums of c ln c in float64 in the order below, the entropies and the MI.
// Order of the float64 sums (it depends on nb alone): JOINT -- thread t of 256 adds the terms of the cells t, t + 256, t + 512, ... of the
// flat index ba * nb + bg in increasing order, starting from 0.0 (a zero cell adds 0.0); the 256 partial sums are then folded as a binary
// tree, v[t] += v[t + s] for s = 128, 64, ..., 1.  MARGINALS -- one thread each, the nb terms in increasing bin order from 0.0.
// Every sum that crosses threads before that is an integer: hist and counts depend on nothing but the sample's own rows.
#include "cmr_sample.h"

namespace {

constexpr int PMI_THREADS = 256;
constexpr int PMI_SLICE = 4096;                 // rows per workgroup
constexpr int PMI_ROWS = PMI_SLICE / PMI_THREADS;
constexpr int PMI_AHEAD = 4;                    // rows of a thread whose pixel loads are in flight together
constexpr int PMI_MAX_BINS = 64;
constexpr int PMI_MAX_CHUNK = 8;                // poses per workgroup at nb <= 32
constexpr int PMI_LDS_BYTES = 32 * 1024;        // the chunk's histograms: 8 poses at nb <= 32, 2 at nb = 64
static_assert(PMI_ROWS % PMI_AHEAD == 0 && PMI_MAX_BINS * PMI_MAX_BINS * 4 <= PMI_LDS_BYTES, "row groups and one histogram in LDS");

inline int pmi_chunk(int nb) {
  const int fit = PMI_LDS_BYTES / (nb * nb * 4);
  return fit > PMI_MAX_CHUNK ? PMI_MAX_CHUNK : fit;
}

// min(nb - 1, max(0, (int)floorf((x - lo) * scale))) for a finite x: the difference and the product rounded one by one (no fma), the
// clamp taken on the float (the same integer, and an overflowed product never reaches the conversion).
__device__ __forceinline__ int pmi_bin(float x, float lo, float scale, float top) {
#pragma clang fp contract(off)
  const float d = x - lo;
  const float m = d * scale;
  return (int)fminf(fmaxf(floorf(m), 0.f), top);
}

__global__ __launch_bounds__(PMI_THREADS) void pmi_fill_kernel(int32_t* __restrict__ hist, int64_t cells, int32_t* __restrict__ counts,
                                                               int ncounts, int32_t* __restrict__ selected, int B) {
  const int64_t i = (int64_t)blockIdx.x * PMI_THREADS + threadIdx.x, stride = (int64_t)gridDim.x * PMI_THREADS;
  const int64_t nvec = cells >> 2;
  int4* hv = reinterpret_cast<int4*>(hist);                              // 16-byte aligned
  for (int64_t v = i; v < nvec; v += stride) hv[v] = make_int4(0, 0, 0, 0);
  if (i < (cells & 3)) hist[(nvec << 2) + i] = 0;
  for (int64_t c = i; c < ncounts; c += stride) counts[c] = 0;
  for (int64_t c = i; c < B; c += stride) selected[c] = 0;
}

template <bool BILINEAR>
__global__ __launch_bounds__(PMI_THREADS) void pmi_hist_kernel(const float* __restrict__ pts, const float* __restrict__ attr,
                                                               const void* __restrict__ mask, int mask_bytes,
                                                               const float* __restrict__ poses, const float* __restrict__ Kin,
                                                               const float* __restrict__ grey, int B, int N, int P, int H, int W, int nb,
                                                               float a_lo, float a_scale, float g_lo, float g_scale, int chunk, int nchunk,
                                                               int nslice, int32_t* __restrict__ hist, int32_t* __restrict__ counts,
                                                               int32_t* __restrict__ selected) {
  extern __shared__ int lh[];                                            // [chunk][nb][nb]
  __shared__ int lview[PMI_MAX_CHUNK];
  __shared__ int part[1][PMI_THREADS / 64];
  // sample fastest: with B a multiple of 8 the workgroups of one sample land on one XCD and share its L2 copy of the sample's image
  const int b = blockIdx.x % B, rest = blockIdx.x / B, c = rest % nchunk, s = rest / nchunk;
  const int tid = threadIdx.x;
  const int p0 = c * chunk;
  const int np = P - p0 < chunk ? P - p0 : chunk;
  const int cells = nb * nb;
  const float top = (float)(nb - 1);
  for (int i = tid; i < np * cells; i += PMI_THREADS) lh[i] = 0;
  if (tid < PMI_MAX_CHUNK) lview[tid] = 0;

  // the thread's rows: registers across the chunk's poses
  float X[PMI_ROWS], Y[PMI_ROWS], Z[PMI_ROWS];
  int code[PMI_ROWS];
  const float* x = pts + (int64_t)b * 3 * N;
  int nsel = 0;
#pragma unroll
  for (int k = 0; k < PMI_ROWS; ++k) {
    const int n = s * PMI_SLICE + k * PMI_THREADS + tid;
    const bool sel = n < N && cmr_sel_or_all(mask, mask_bytes, (int64_t)b * N + n);
    X[k] = Y[k] = Z[k] = 0.f;
    code[k] = -2;
    if (sel) {
      X[k] = x[n];
      Y[k] = x[N + n];
      Z[k] = x[2 * N + n];
      const float a = attr[(int64_t)b * N + n];
      code[k] = isfinite(a) ? pmi_bin(a, a_lo, a_scale, top) : -1;
      ++nsel;
    }
  }
  __syncthreads();

  const float* K = Kin + 9 * b;
  const float* img = grey + (int64_t)b * H * W;
  for (int pp = 0; pp < np; ++pp) {                                      // workgroup-uniform
    const float* Pp = poses + ((int64_t)b * P + p0 + pp) * 16;
    int* lhp = lh + pp * cells;
    int nview = 0;
#pragma unroll
    for (int k0 = 0; k0 < PMI_ROWS; k0 += PMI_AHEAD) {
      CmrTaps tp[PMI_AHEAD];
      bool view[PMI_AHEAD];
      float t[PMI_AHEAD][4];
#pragma unroll
      for (int u = 0; u < PMI_AHEAD; ++u) {
        const CmrProj pr = cmr_project_select(Pp, K, X[k0 + u], Y[k0 + u], Z[k0 + u], H, W, 0.f);
        view[u] = pr.view && code[k0 + u] > -2;
        tp[u] = cmr_taps<BILINEAR>(pr, view[u] && code[k0 + u] >= 0, H, W);
        nview += view[u] ? 1 : 0;
      }
#pragma unroll
      for (int u = 0; u < PMI_AHEAD; ++u) {
        t[u][0] = img[tp[u].o00];
        t[u][1] = t[u][2] = t[u][3] = 0.f;
        if (BILINEAR) { t[u][1] = img[tp[u].o01]; t[u][2] = img[tp[u].o10]; t[u][3] = img[tp[u].o11]; }
      }
#pragma unroll
      for (int u = 0; u < PMI_AHEAD; ++u) {
        const float g = cmr_tap_value<BILINEAR>(tp[u], t[u][0], t[u][1], t[u][2], t[u][3]);
        if (view[u] && code[k0 + u] >= 0 && isfinite(g)) atomicAdd(&lhp[code[k0 + u] * nb + pmi_bin(g, g_lo, g_scale, top)], 1);
      }
    }
    // in-view rows of the wave -> the pose's LDS word
    for (int o = 32; o > 0; o >>= 1) nview += __shfl_xor(nview, o);
    if ((tid & 63) == 0 && nview) atomicAdd(&lview[pp], nview);
  }
  __syncthreads();

  int32_t* hb = hist + ((int64_t)b * P + p0) * cells;
  if (nslice == 1) {
    for (int i = tid; i < np * cells; i += PMI_THREADS)
      if (lh[i]) hb[i] = lh[i];
    if (tid < np && lview[tid]) counts[2 * ((int64_t)b * P + p0 + tid)] = lview[tid];
  } else {
    for (int i = tid; i < np * cells; i += PMI_THREADS)
      if (lh[i]) atomicAdd(&hb[i], lh[i]);
    if (tid < np && lview[tid]) atomicAdd(&counts[2 * ((int64_t)b * P + p0 + tid)], lview[tid]);
  }
  if (c == 0) {                                                          // workgroup-uniform
    for (int o = 32; o > 0; o >>= 1) nsel += __shfl_xor(nsel, o);
    if ((tid & 63) == 0) part[0][tid >> 6] = nsel;
    __syncthreads();
    const int tot = part[0][0] + part[0][1] + part[0][2] + part[0][3];
    if (tid == 0 && tot) atomicAdd(&selected[b], tot);
  }
}

__device__ __forceinline__ double pmi_clogc(int c) { return c > 0 ? (double)c * log((double)c) : 0.0; }

__global__ __launch_bounds__(PMI_THREADS) void pmi_final_kernel(const int32_t* __restrict__ hist, int nb, int32_t* __restrict__ counts,
                                                                double* __restrict__ entropy, double* __restrict__ mi) {
  __shared__ int h[PMI_MAX_BINS * PMI_MAX_BINS];
  __shared__ int ma[PMI_MAX_BINS], mg[PMI_MAX_BINS];
  __shared__ double v[PMI_THREADS];
  __shared__ double sm[2];
  const int64_t bp = blockIdx.x;
  const int tid = threadIdx.x, cells = nb * nb;
  const int32_t* hp = hist + bp * cells;
  double acc = 0.0;
  for (int i = tid; i < cells; i += PMI_THREADS) {                       // cells t, t + 256, ... in increasing order
    const int cnt = hp[i];
    h[i] = cnt;
    acc += pmi_clogc(cnt);
  }
  v[tid] = acc;
  __syncthreads();
  if (tid < nb) {                                                        // marginal of the attribute: row sums
    int sum = 0;
    for (int j = 0; j < nb; ++j) sum += h[tid * nb + j];
    ma[tid] = sum;
  } else if (tid >= 64 && tid < 64 + nb) {                               // marginal of the grey value: column sums
    int sum = 0;
    for (int j = 0; j < nb; ++j) sum += h[j * nb + (tid - 64)];
    mg[tid - 64] = sum;
  }
  for (int st = PMI_THREADS / 2; st > 0; st >>= 1) {                     // the binary tree over the 256 partial sums
    if (tid < st) v[tid] += v[tid + st];
    __syncthreads();
  }
  if (tid == 0 || tid == 64) {                                           // the nb terms in increasing bin order
    const int* m = tid == 0 ? ma : mg;
    double sum = 0.0;
    for (int j = 0; j < nb; ++j) sum += pmi_clogc(m[j]);
    sm[tid >> 6] = sum;
  }
  __syncthreads();
  if (tid == 0) {
    int n = 0;
    for (int j = 0; j < nb; ++j) n += ma[j];
    double ha = 0.0, hg = 0.0, hag = 0.0;
    if (n > 0) {
      const double ln = log((double)n), dn = (double)n;
      ha = ln - sm[0] / dn;
      hg = ln - sm[1] / dn;
      hag = ln - v[0] / dn;
    }
    counts[2 * bp + 1] = n;
    entropy[3 * bp] = ha;
    entropy[3 * bp + 1] = hg;
    entropy[3 * bp + 2] = hag;
    mi[bp] = (ha + hg) - hag;
  }
}

}  // namespace

extern "C" int cmr_pose_mi_f32(const float* pts, const float* attr, const void* mask, int mask_bytes, const float* poses, int P,
                               const float* K, const float* grey, int B, int N, int H, int W, int mode, int bins, float a_lo, float a_hi,
                               float g_lo, float g_hi, int32_t* hist, int32_t* counts, int32_t* selected, double* entropy, double* mi,
                               hipStream_t stream) {
  CMR_REQUIRE(pts && attr && poses && K && grey && hist && counts && selected && entropy && mi);
  CMR_REQUIRE(cmr_cloud_map_ok(B, N, H, W) && P > 0 && P <= CMR_MAX_POSES);
  CMR_REQUIRE((mask_bytes == 1 || mask_bytes == 8) && (mode == 0 || mode == 1) && bins >= 2 && bins <= PMI_MAX_BINS);
  CMR_REQUIRE(__builtin_isfinite(a_lo) && __builtin_isfinite(a_hi) && a_lo < a_hi && __builtin_isfinite(g_lo) && __builtin_isfinite(g_hi) &&
              g_lo < g_hi);
  CMR_REQUIRE(cmr_aligned16(hist));
  // nb / (hi - lo) in double, rounded once
  const float a_scale = (float)((double)bins / ((double)a_hi - (double)a_lo)), g_scale = (float)((double)bins / ((double)g_hi - (double)g_lo));
  CMR_REQUIRE(__builtin_isfinite(a_scale) && __builtin_isfinite(g_scale));
  const int chunk = pmi_chunk(bins), nchunk = (P + chunk - 1) / chunk, nslice = (N + PMI_SLICE - 1) / PMI_SLICE;
  const int64_t groups = (int64_t)nslice * nchunk * B;
  CMR_REQUIRE(groups <= 0x7fffffff);
  const int64_t cells = (int64_t)B * P * bins * bins;
  hipLaunchKernelGGL(pmi_fill_kernel, dim3(cmr_fill_blocks(cells / 4, PMI_THREADS)), dim3(PMI_THREADS), 0, stream, hist, cells, counts,
                     2 * B * P, selected, B);
  const size_t lds = (size_t)chunk * bins * bins * 4;
  if (mode == 1)
    hipLaunchKernelGGL(pmi_hist_kernel<true>, dim3((unsigned)groups), dim3(PMI_THREADS), lds, stream, pts, attr, mask, mask_bytes, poses, K,
                       grey, B, N, P, H, W, bins, a_lo, a_scale, g_lo, g_scale, chunk, nchunk, nslice, hist, counts, selected);
  else
    hipLaunchKernelGGL(pmi_hist_kernel<false>, dim3((unsigned)groups), dim3(PMI_THREADS), lds, stream, pts, attr, mask, mask_bytes, poses, K,
                       grey, B, N, P, H, W, bins, a_lo, a_scale, g_lo, g_scale, chunk, nchunk, nslice, hist, counts, selected);
  hipLaunchKernelGGL(pmi_final_kernel, dim3((unsigned)(B * P)), dim3(PMI_THREADS), 0, stream, (const int32_t*)hist, bins, counts, entropy, mi);
  return cmr_launch_status();
}
