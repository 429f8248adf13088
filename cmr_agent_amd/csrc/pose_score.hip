// Pose scoring (port extension): for P candidate poses per sample, the truncated feature-metric cost of the selected points
// against the pixel features -- per pose and row exactly the quantity cmr_guided_match_f32 (guided_match.hip) calls `dist`,
// clamped at tau, squared and summed in float64.  One sweep scores all P poses: a row's feature stays in registers across the poses.
//
// Two launches on the caller's stream, no memset, no atomics, whatever P is:
//   ps_score_kernel  grid (row slices x pose chunks x B, the sample fastest): a workgroup owns PS_SLICE consecutive rows of one sample
//                    and PS_CHUNK consecutive poses.  It first packs the slice's SELECTED rows, in increasing n, into a list in LDS
//                    (ballot + prefix over the four waves), so the work follows the selected rows.  Then a 16-lane group per listed row
//                    (group g takes list entries g, g + 16, ...): lane j keeps channels 4j .. 4j+3 of the point feature in registers and
//                    the group walks the chunk's poses PS_AHEAD at a time -- projection (cmr_project.h, the form without branches; the pose
//                    index is wave-uniform, so R, t and K arrive through scalar loads), then the window offsets in increasing p with the
//                    PS_AHEAD poses' pixel rows loaded together, the direct sum of squared differences and the 16-lane DPP butterfly,
//                    minimum kept with a strict <.  A row that is not in view reads a clamped address and costs a select, not a branch;
//                    every loop bound is wave-uniform, so EXEC stays full under the DPP moves.  Lane j of the group accumulates the
//                    poses j, j + 16 of the chunk (float64 cost, packed integer counts) in registers; at the end the 16 groups' sums
//                    are added IN GROUP ORDER into the slot of (b, p, slice) in the workspace.
//   ps_final_kernel  a thread per (b, p): adds the slots IN SLICE ORDER -> score, counts; the thread of p = 0 adds the slices' sizes ->
//                    selected.
// Summation order of one score: inside a slice, per group the listed rows g, g + 16, ... in order, then the groups 0 .. 15 in order; then
// the slices in order.  The list depends only on the sample's own mask, PS_SLICE is a constant, and a pose's place in its chunk decides
// only WHICH lane adds, never the order: the sum does not depend on B, on P, on the pose's index or on how the poses are chunked.
#include "cmr_project.h"

namespace {

constexpr int PS_C = 64;            // feature width (the model's only one)
constexpr int PS_THREADS = 256;     // 4 waves
constexpr int PS_LANES = 16;        // lanes per row: 16 x float4 = one 256-byte feature row
constexpr int PS_GROUPS = PS_THREADS / PS_LANES;
constexpr int PS_SLICE = 256;       // rows per workgroup, one per thread in the packing step.  A constant: the summation order hangs on it
constexpr int PS_CHUNK = 32;        // poses per workgroup: 2 accumulators per lane
constexpr int PS_AHEAD = 4;         // poses whose pixel loads are in flight together per group
static_assert(PS_SLICE == PS_THREADS && PS_CHUNK % PS_LANES == 0 && PS_LANES % PS_AHEAD == 0, "packing and accumulator layout");

__global__ __launch_bounds__(PS_THREADS) void ps_score_kernel(const float* __restrict__ pts, const float* __restrict__ pc,
                                                              const float* __restrict__ img, const void* __restrict__ mask, int mask_bytes,
                                                              const float* __restrict__ poses, const float* __restrict__ Kin, int B, int N,
                                                              int P, int h, int w, int radius, float tau, int nslice, int nchunk,
                                                              double* __restrict__ part, int32_t* __restrict__ cpart,
                                                              int32_t* __restrict__ nsel_ws) {
  __shared__ int list[PS_SLICE];
  __shared__ int wcnt[PS_THREADS / 64];
  __shared__ double sacc[PS_GROUPS][PS_CHUNK];
  __shared__ int scnt[PS_GROUPS][PS_CHUNK];
  // sample fastest: with B a multiple of 8 the workgroups of one sample land on one XCD and share its L2 copy of the sample's map
  const int b = blockIdx.x % B, rest = blockIdx.x / B, chunk = rest % nchunk, s = rest / nchunk;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the slice's selected rows, in increasing n
  const int n0 = s * PS_SLICE + tid;
  const bool sel = n0 < N && cmr_sel(mask, mask_bytes, (int64_t)b * N + n0);
  const unsigned long long bal = __ballot(sel);
  if (lane == 0) wcnt[wave] = __popcll(bal);
  __syncthreads();
  int base = 0;
  for (int i = 0; i < wave; ++i) base += wcnt[i];
  const int nsel = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
  if (sel) list[base + __popcll(bal & ((1ull << lane) - 1ull))] = n0;
  __syncthreads();

  const int grp = tid >> 4, j = tid & 15;
  const int p0 = chunk * PS_CHUNK;
  const int np = P - p0 < PS_CHUNK ? P - p0 : PS_CHUNK;
  const float* K = Kin + 9 * b;
  const float* Pb = poses + ((int64_t)b * P + p0) * 16;
  const float* x = pts + (int64_t)b * 3 * N;
  const float4* img_b = reinterpret_cast<const float4*>(img + (int64_t)b * h * w * PS_C) + j;
  const int total = (2 * radius + 1) * (2 * radius + 1);
  const float r = (float)radius;
  double acc[PS_CHUNK / PS_LANES] = {};
  int cacc[PS_CHUNK / PS_LANES] = {};              // in view (low half) and close (high half): at most 16 rows per group
  for (int q0 = 0; q0 < nsel; q0 += PS_GROUPS) {   // wave-uniform: a group past the list scores the list's first row and drops it
    const int q = q0 + grp;
    const bool active = q < nsel;
    const int n = list[active ? q : 0];
    const float X = x[n], Y = x[N + n], Z = x[2 * N + n];
    const float4 a = reinterpret_cast<const float4*>(pc + ((int64_t)b * N + n) * PS_C)[j];
#pragma unroll
    for (int kk = 0; kk < PS_CHUNK / PS_LANES; ++kk) {
      for (int m = 0; m < PS_LANES / PS_AHEAD; ++m) {
        const int pb = kk * PS_LANES + m * PS_AHEAD;
        if (pb >= np) break;                       // wave-uniform
        int cxi[PS_AHEAD], cyi[PS_AHEAD];
        bool view[PS_AHEAD];
        float best[PS_AHEAD];
#pragma unroll
        for (int u = 0; u < PS_AHEAD; ++u) {
          // a pose past the chunk's end repeats the last one
          const CmrProj pr = cmr_project_select(Pb + 16 * (pb + u < np ? pb + u : np - 1), K, X, Y, Z, h, w, r);
          view[u] = pr.view;
          cxi[u] = pr.cx;
          cyi[u] = pr.cy;
          best[u] = __builtin_huge_valf();
        }
        // the window offsets in increasing p (dy outer, dx inner); per offset the PS_AHEAD poses' loads are issued together, then scored
        int dx = -radius, dy = -radius;            // wave-uniform
        for (int k = 0; k < total; ++k) {
          float4 f[PS_AHEAD];
          bool in[PS_AHEAD];
#pragma unroll
          for (int u = 0; u < PS_AHEAD; ++u) {
            const int px = cxi[u] + dx, py = cyi[u] + dy;
            in[u] = (px >= 0) & (px < w) & (py >= 0) & (py < h);
            const int p = (py < 0 ? 0 : (py >= h ? h - 1 : py)) * w + (px < 0 ? 0 : (px >= w ? w - 1 : px));
            f[u] = img_b[(int64_t)p * (PS_C / 4)];
          }
          __builtin_amdgcn_sched_barrier(0);       // all PS_AHEAD loads are issued before the first score waits for one
#pragma unroll
          for (int u = 0; u < PS_AHEAD; ++u) {
            const float d0 = a.x - f[u].x, d1 = a.y - f[u].y, d2 = a.z - f[u].z, d3 = a.w - f[u].w;
            float sc = d0 * d0;
            sc = fmaf(d1, d1, sc);
            sc = fmaf(d2, d2, sc);
            sc = fmaf(d3, d3, sc);
            sc = cmr_sum16(sc);
            best[u] = fminf(best[u], in[u] ? sc : __builtin_huge_valf());      // a pixel outside the map is scored and dropped; a NaN score never wins
          }
          if (++dx > radius) { dx = -radius; ++dy; }
        }
#pragma unroll
        for (int u = 0; u < PS_AHEAD; ++u) {
          const float dist = sqrtf(best[u]);                             // +inf for a window without a finite score
          const float d = view[u] ? fminf(dist, tau) : tau;
          const bool close = view[u] && dist <= tau;
          const bool mine = active && j == m * PS_AHEAD + u && pb + u < np;
          acc[kk] += mine ? (double)d * (double)d : 0.0;
          cacc[kk] += mine ? (int)view[u] + ((int)close << 16) : 0;
        }
      }
    }
  }
#pragma unroll
  for (int kk = 0; kk < PS_CHUNK / PS_LANES; ++kk) {
    sacc[grp][kk * PS_LANES + j] = acc[kk];
    scnt[grp][kk * PS_LANES + j] = cacc[kk];
  }
  __syncthreads();
  if (tid < np) {
    double v = sacc[0][tid];
    int c = scnt[0][tid];
    for (int g = 1; g < PS_GROUPS; ++g) { v += sacc[g][tid]; c += scnt[g][tid]; }      // group order
    const int64_t slot = ((int64_t)b * P + p0 + tid) * nslice + s;
    part[slot] = v;
    cpart[2 * slot] = c & 0xffff;
    cpart[2 * slot + 1] = c >> 16;
  }
  if (chunk == 0 && tid == 0) nsel_ws[(int64_t)b * nslice + s] = nsel;
}

__global__ __launch_bounds__(256) void ps_final_kernel(int B, int P, int nslice, const double* __restrict__ part,
                                                       const int32_t* __restrict__ cpart, const int32_t* __restrict__ nsel_ws,
                                                       double* __restrict__ score, int32_t* __restrict__ counts,
                                                       int32_t* __restrict__ selected) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * P) return;
  double v = 0.0;
  int c0 = 0, c1 = 0;
  for (int s = 0; s < nslice; ++s) {                                     // slice order
    v += part[i * nslice + s];
    c0 += cpart[2 * (i * nslice + s)];
    c1 += cpart[2 * (i * nslice + s) + 1];
  }
  score[i] = v;
  counts[2 * i] = c0;
  counts[2 * i + 1] = c1;
  if (i % P == 0) {
    const int64_t b = i / P;
    int n = 0;
    for (int s = 0; s < nslice; ++s) n += nsel_ws[b * nslice + s];
    selected[b] = n;
  }
}

struct PsWs { int64_t part, cpart, nsel, total; };

inline PsWs ps_layout(int B, int N, int P) {
  PsWs L;
  const int64_t nslice = ((int64_t)N + PS_SLICE - 1) / PS_SLICE;
  L.part = 0;
  L.cpart = L.part + cmr_up16((int64_t)B * P * nslice * 8);
  L.nsel = L.cpart + cmr_up16((int64_t)B * P * nslice * 8);
  L.total = L.nsel + cmr_up16((int64_t)B * nslice * 4);
  return L;
}

}  // namespace

extern "C" int64_t cmr_pose_score_workspace_bytes(int B, int N, int P) {
  return B <= 0 || N <= 0 || P <= 0 ? 0 : ps_layout(B, N, P).total;
}

extern "C" int cmr_pose_score_f32(const float* pts, const float* pc_feat, const float* img_feat, int C, int B, int N, int h, int w,
                                  const void* mask, int mask_bytes, const float* poses, int P, const float* K, int radius, float tau,
                                  double* score, int32_t* counts, int32_t* selected, void* workspace, int64_t workspace_bytes,
                                  hipStream_t stream) {
  CMR_REQUIRE(pts && pc_feat && img_feat && mask && poses && K && score && counts && selected && workspace);
  CMR_REQUIRE(C == PS_C && cmr_cloud_map_ok(B, N, h, w) && P > 0 && P <= CMR_MAX_POSES);
  CMR_REQUIRE(mask_bytes == 1 || mask_bytes == 8);
  CMR_REQUIRE(radius >= 0 && radius <= CMR_MAX_RADIUS && tau > 0.f && __builtin_isfinite(tau));
  CMR_REQUIRE(cmr_aligned16(pc_feat) && cmr_aligned16(img_feat) && cmr_aligned16(workspace));
  CMR_REQUIRE(workspace_bytes >= cmr_pose_score_workspace_bytes(B, N, P));
  const int nslice = (N + PS_SLICE - 1) / PS_SLICE, nchunk = (P + PS_CHUNK - 1) / PS_CHUNK;
  const int64_t groups = (int64_t)nslice * nchunk * B;
  CMR_REQUIRE(groups <= 0x7fffffff);
  const PsWs L = ps_layout(B, N, P);
  double* part = (double*)((char*)workspace + L.part);
  int32_t* cpart = (int32_t*)((char*)workspace + L.cpart);
  int32_t* nsel = (int32_t*)((char*)workspace + L.nsel);
  hipLaunchKernelGGL(ps_score_kernel, dim3((unsigned)groups), dim3(PS_THREADS), 0, stream, pts, pc_feat, img_feat, mask, mask_bytes, poses, K,
                     B, N, P, h, w, radius, tau, nslice, nchunk, part, cpart, nsel);
  hipLaunchKernelGGL(ps_final_kernel, dim3((unsigned)(((int64_t)B * P + 255) / 256)), dim3(256), 0, stream, B, P, nslice,
                     (const double*)part, (const int32_t*)cpart, (const int32_t*)nsel, score, counts, selected);
  return cmr_launch_status();
}
