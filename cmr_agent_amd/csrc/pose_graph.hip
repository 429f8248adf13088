// A pose-graph solve over a chain of poses and its loop edges (port extension): Gauss-Newton on the relative-pose
// residuals, the linear system solved matrix-free by preconditioned conjugate gradients, the whole loop on the device.  The contract --
// residual, Jacobian, Huber, the sums' orders -- is include/cmr_hip.h's.
//
//   cmr_pose_graph_linearize_f64   pg_linearize_kernel (one edge per lane) + pg_total_kernel (the workgroups' slots in slot order)
//   cmr_pose_graph_optimize_f64    launches, all on the caller's stream, 2 (iters + 1) + iters (2 + 2 cg_iters) + 2 whatever the data:
//     pg_init_kernel       poses -> the float64 working poses (buffer 0 of two); trace = 0; state;
//     for k = 0 .. iters:
//       pg_linearize_kernel  the terms of every edge at the CANDIDATE poses (k = 0: the given ones; else what step k - 1 wrote into the
//                            other buffer), the cost through per-workgroup slots;
//       pg_begin_kernel      one workgroup, the only writer of the loop's state: adds the cost slots in slot order and judges step k - 1 --
//                            within the tolerances: the buffers flip and the loop stops; else cost not below: the candidate is dropped
//                            (the buffers are not flipped: that is the undo) and the loop stops; else the buffers flip;
//       (k < iters:)
//       pg_blocks_kernel     one node per lane walks its incidence: M_n, its inverse through cmr_pnp_chol6, g_n, x = 0, r = -g, z = M^-1 r;
//       for c = 0 .. cg_iters - 1:
//         pg_apply_kernel    beta and p = z + beta p (its own and its neighbours', from the other p buffer), q = H p, the p.q slots;
//         pg_update_kernel   alpha, x += alpha p, r -= alpha q, z = M^-1 r, the r.z slots;
//       pg_step_kernel       X_n <- [Exp(dw_n) | dv_n] X_n into the other buffer, the largest |dw|, |dv| per workgroup, the trace row's CG part;
//     pg_final_kernel      the accepted poses as [4][4], cost, status.
// alpha, beta and the CG stop are recomputed by EVERY workgroup from the slots in slot order: the same bits everywhere, no launch of one
// workgroup between the two kernels of an iteration.  A call that has stopped -- the outer loop, or CG inside an outer iteration -- turns
// its remaining launches into early returns read from its state in the workspace.  No atomics; every slot, flag and output has one writer,
// and no kernel reads a flag that a workgroup of the same launch writes (pg_apply reads done_b and writes done_a, pg_update the reverse).
// The working pose's left update, Rodrigues and the 6 x 6 Cholesky are cmr_pnp.h's, and so is the slot-order sum: the node and edge slots
// are laid out with its stride (CMR_GN_NACC doubles per workgroup, one entry per quantity).
#include <cmath>

#include "cmr_pnp.h"

namespace {

constexpr int PG_T = 256;                   // lanes per workgroup: one edge or one node each.  A constant: the sums' orders rest on it
constexpr int PG_NS = CMR_GN_NACC;          // doubles per workgroup slot (cmr_slot_sum's stride)
// a slot's entries.  Q_RZ and Q_RZ + 1 alternate: CG iteration c reads r.z at Q_RZ + (c & 1) and writes the next at Q_RZ + ((c + 1) & 1)
enum { Q_COST = 0, Q_PQ = 1, Q_RZ = 2, Q_RZ0 = 4, Q_SING = 5, Q_BAD = 6, Q_MAXW = 7, Q_MAXV = 8 };

struct PgState {
  double cost_prev;                         // the cost at the accepted poses
  int32_t stop, code, executed, which;      // which: the buffer that holds the accepted poses
  int32_t done_a, used_a, done_b, used_b;   // CG of this outer iteration has stopped (a: converged, seen by pg_apply; b: what pg_update tells pg_apply)
  int32_t wide, pad;
};

// the workgroup's sum, valid in every thread: the butterfly of cmr_wave_sum_d, then the four waves in wave order.  Every thread calls it.
__device__ __forceinline__ double pg_block_sum(double v, double (&sm)[PG_T / 64]) {
  v = cmr_wave_sum_d(v);
  __syncthreads();                          // the previous call's readers are done
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sm[0] + sm[1]) + sm[2]) + sm[3];
}
__device__ __forceinline__ double pg_block_max(double v, double (&sm)[PG_T / 64]) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmax(fmax(sm[0], sm[1]), fmax(sm[2], sm[3]));
}

// pose n as R (row-major) and t: LD = 16 from a row-major [4][4], LD = 12 from a working pose
template <int LD>
__device__ __forceinline__ void pg_pose(const double* __restrict__ P, int64_t n, double (&R)[9], double (&t)[3]) {
  const double* p = P + n * LD;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) R[3 * i + j] = LD == 16 ? p[4 * i + j] : p[3 * i + j];
    t[i] = LD == 16 ? p[4 * i + 3] : p[9 + i];
  }
}

// entry (i, j), i <= j, of a symmetric 6 x 6 kept as its 21 upper entries row by row
__host__ __device__ constexpr int pg_up(int i, int j) { return 6 * i - i * (i - 1) / 2 + (j - i); }

// o = S v for such a matrix
__device__ __forceinline__ void pg_symv(const double (&S)[21], const double (&v)[6], double (&o)[6]) {
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) s += S[i <= j ? pg_up(i, j) : pg_up(j, i)] * v[j];
    o[i] = s;
  }
}

// One edge's terms as the header states them.  -> whether the edge is wide.
__device__ __forceinline__ bool pg_terms(const double (&Ri)[9], const double (&ti)[3], const double (&Rj)[9], const double (&tj)[3],
                                         const double (&Rz)[9], const double (&tz)[3], double w_rot, double w_trans, double huber,
                                         double (&res)[6], double& chi, double& scale, double& cost, double (&A)[21], double (&b)[6]) {
  double B[9], RD[9];                                             // B = Rz^T Rj^T, RD = B Ri
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c) B[3 * a + c] = Rz[a] * Rj[3 * c] + Rz[3 + a] * Rj[3 * c + 1] + Rz[6 + a] * Rj[3 * c + 2];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c) RD[3 * a + c] = B[3 * a] * Ri[c] + B[3 * a + 1] * Ri[3 + c] + B[3 * a + 2] * Ri[6 + c];
  const double d[3] = {ti[0] - tj[0], ti[1] - tj[1], ti[2] - tj[2]};
  double u[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) u[a] = (Rj[a] * d[0] + Rj[3 + a] * d[1] + Rj[6 + a] * d[2]) - tz[a];
#pragma unroll
  for (int a = 0; a < 3; ++a) res[3 + a] = Rz[a] * u[0] + Rz[3 + a] * u[1] + Rz[6 + a] * u[2];
  // Log from the antisymmetric part
  const double ax = 0.5 * (RD[7] - RD[5]), ay = 0.5 * (RD[2] - RD[6]), az = 0.5 * (RD[3] - RD[1]);
  const double s2 = ax * ax + ay * ay + az * az, s = sqrt(s2), c = 0.5 * ((RD[0] + RD[4] + RD[8]) - 1.0);
  const double th = atan2(s, c);
  const double f = s < 1e-8 ? 1.0 + s2 / 6.0 : th / s;
  res[0] = f * ax;
  res[1] = f * ay;
  res[2] = f * az;
  const double k = th < 1e-4 ? 1.0 / 12.0 : 1.0 / (th * th) - (1.0 + cos(th)) / (2.0 * th * sin(th));
  // Jr^-1 = I + 1/2 [phi]x + k [phi]x^2,  [phi]x^2 = phi phi^T - |phi|^2 I
  const double p0 = res[0], p1 = res[1], p2 = res[2], pp = p0 * p0 + p1 * p1 + p2 * p2;
  const double Ji[9] = {1.0 + k * (p0 * p0 - pp), -0.5 * p2 + k * p0 * p1,      0.5 * p1 + k * p0 * p2,
                        0.5 * p2 + k * p0 * p1,   1.0 + k * (p1 * p1 - pp),     -0.5 * p0 + k * p1 * p2,
                        -0.5 * p1 + k * p0 * p2,  0.5 * p0 + k * p1 * p2,       1.0 + k * (p2 * p2 - pp)};
  // J = [[Ja, 0], [Jc, B]],  Ja = Jr^-1 Ri^T,  Jc = -B [ti]x
  double Ja[9], Jc[9];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int q = 0; q < 3; ++q) Ja[3 * a + q] = Ji[3 * a] * Ri[3 * q] + Ji[3 * a + 1] * Ri[3 * q + 1] + Ji[3 * a + 2] * Ri[3 * q + 2];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    Jc[3 * a] = -(B[3 * a + 1] * ti[2] - B[3 * a + 2] * ti[1]);
    Jc[3 * a + 1] = -(B[3 * a + 2] * ti[0] - B[3 * a] * ti[2]);
    Jc[3 * a + 2] = -(B[3 * a] * ti[1] - B[3 * a + 1] * ti[0]);
  }
  const double chi2 = w_rot * pp + w_trans * (res[3] * res[3] + res[4] * res[4] + res[5] * res[5]);
  chi = sqrt(chi2);
  const bool outer = huber > 0.0 && chi > huber;
  scale = outer ? huber / chi : 1.0;
  {                                                               // from the ROUNDED chi, unfused: the edge's cost follows from its chi bit for bit
#pragma clang fp contract(off)
    cost = outer ? huber * chi - (0.5 * huber) * huber : (0.5 * chi) * chi;
  }
  const double sr = scale * w_rot, st = scale * w_trans;
  // A = s J^T W J, b = s J^T W r: column r of J is (Ja[.][r], Jc[.][r]) for r < 3 and (0, B[.][r - 3]) above
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int q = r; q < 3; ++q)
      A[pg_up(r, q)] = sr * (Ja[r] * Ja[q] + Ja[3 + r] * Ja[3 + q] + Ja[6 + r] * Ja[6 + q]) +
                       st * (Jc[r] * Jc[q] + Jc[3 + r] * Jc[3 + q] + Jc[6 + r] * Jc[6 + q]);
#pragma unroll
    for (int q = 0; q < 3; ++q) A[pg_up(r, 3 + q)] = st * (Jc[r] * B[q] + Jc[3 + r] * B[3 + q] + Jc[6 + r] * B[6 + q]);
    b[r] = sr * (Ja[r] * res[0] + Ja[3 + r] * res[1] + Ja[6 + r] * res[2]) + st * (Jc[r] * res[3] + Jc[3 + r] * res[4] + Jc[6 + r] * res[5]);
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int q = r; q < 3; ++q) A[pg_up(3 + r, 3 + q)] = st * (B[r] * B[q] + B[3 + r] * B[3 + q] + B[6 + r] * B[6 + q]);
    b[3 + r] = st * (B[r] * res[3] + B[3 + r] * res[4] + B[6 + r] * res[5]);
  }
  return th > 3.0;
}

// One edge per lane.  st = null: the public entry on [4][4] poses.  Else the loop's: the candidate poses are those of buffer which ^ cand.
// An edge whose indices do not name two different poses gets zero terms.  r, chi and scale may be null.
template <int LD>
__global__ __launch_bounds__(PG_T) void pg_linearize_kernel(const double* __restrict__ poses, const PgState* __restrict__ st, int cand, int64_t F,
                                                            const int32_t* __restrict__ edges, const double* __restrict__ meas,
                                                            const double* __restrict__ weights, int64_t E, double huber,
                                                            double* __restrict__ r, double* __restrict__ chi, double* __restrict__ scale,
                                                            double* __restrict__ A, double* __restrict__ b, double* __restrict__ slots,
                                                            int32_t* __restrict__ wslots) {
  __shared__ double sm[PG_T / 64];
  __shared__ int part[1][PG_T / 64];
  if (st) {
    if (st->stop) return;
    poses += (int64_t)(st->which ^ cand) * F * 12;
  }
  const int64_t e = (int64_t)blockIdx.x * PG_T + threadIdx.x;
  double res[6] = {}, ch = 0.0, sc = 0.0, co = 0.0, Ae[21] = {}, be[6] = {};
  bool wide = false;
  if (e < E) {
    const int64_t i = edges[2 * e], j = edges[2 * e + 1];
    if (i >= 0 && i < F && j >= 0 && j < F && i != j) {
      double Ri[9], ti[3], Rj[9], tj[3], Rz[9], tz[3];
      pg_pose<LD>(poses, i, Ri, ti);
      pg_pose<LD>(poses, j, Rj, tj);
      pg_pose<16>(meas, e, Rz, tz);
      wide = pg_terms(Ri, ti, Rj, tj, Rz, tz, weights[2 * e], weights[2 * e + 1], huber, res, ch, sc, co, Ae, be);
    }
    if (r) {
#pragma unroll
      for (int q = 0; q < 6; ++q) r[6 * e + q] = res[q];
      chi[e] = ch;
      scale[e] = sc;
    }
#pragma unroll
    for (int q = 0; q < 21; ++q) A[21 * e + q] = Ae[q];
#pragma unroll
    for (int q = 0; q < 6; ++q) b[6 * e + q] = be[q];
  }
  const double total = pg_block_sum(co, sm);
  const bool flag[1] = {wide};
  int count[1];
  cmr_block_counts<1, PG_T>(flag, part, count);
  if (threadIdx.x == 0) {
    slots[(int64_t)blockIdx.x * PG_NS + Q_COST] = total;
    wslots[blockIdx.x] = count[0];
  }
}

// the public linearisation's totals: the slots in slot order
__global__ __launch_bounds__(64) void pg_total_kernel(const double* __restrict__ slots, const int32_t* __restrict__ wslots, int nwg,
                                                      double* __restrict__ cost, int32_t* __restrict__ wide) {
  if (threadIdx.x == 0) cost[0] = cmr_slot_sum(slots, nwg, Q_COST);
  if (threadIdx.x == 1) {
    int64_t w = 0;
    for (int s = 0; s < nwg; ++s) w += wslots[s];
    wide[0] = (int32_t)w;
  }
}

// ---------------------------------------------------------------------------------------------------------------------- the loop
__global__ __launch_bounds__(PG_T) void pg_init_kernel(const double* __restrict__ poses_in, int64_t F, int iters, PgState* __restrict__ st,
                                                       double* __restrict__ buf, double* __restrict__ trace) {
  const int64_t t = (int64_t)blockIdx.x * PG_T + threadIdx.x;
  if (t < (int64_t)iters * 5) trace[t] = 0.0;
  if (t < F) {
    double R[9], tt[3];
    pg_pose<16>(poses_in, t, R, tt);
#pragma unroll
    for (int q = 0; q < 9; ++q) buf[12 * t + q] = R[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) buf[12 * t + 9 + q] = tt[q];
  }
  if (t == 0) {
    st->cost_prev = 0.0;
    st->stop = 0;
    st->code = 1;                           // iterations exhausted, until pg_begin_kernel says otherwise
    st->executed = 0;
    st->which = 0;
    st->done_a = st->used_a = st->done_b = st->used_b = 0;
    st->wide = 0;
    st->pad = 0;
  }
}

// One workgroup, the only writer of stop, code, which and cost_prev.  k = 0: the start (wide edges, a cost that is not finite); k > 0:
// judges step k - 1 from the cost at its candidate poses.
__global__ __launch_bounds__(64) void pg_begin_kernel(int k, int iters, int nwg_e, int nwg_n, double tol_rot, double tol_trans,
                                                      PgState* __restrict__ st, const double* __restrict__ eslots,
                                                      const int32_t* __restrict__ wslots, const double* __restrict__ nslots,
                                                      double* __restrict__ trace) {
  if (threadIdx.x != 0 || st->stop) return;
  const double cost = cmr_slot_sum(eslots, nwg_e, Q_COST);
  if (k == 0) {
    int64_t w = 0;
    for (int s = 0; s < nwg_e; ++s) w += wslots[s];
    st->wide = (int32_t)w;
    st->cost_prev = cost;
    if (w > 0) { st->code = 3; st->stop = 1; return; }
    if (!isfinite(cost)) { st->code = 2; st->stop = 1; return; }
    if (iters > 0) trace[0] = cost;
    return;
  }
  const double sing = cmr_slot_sum(nslots, nwg_n, Q_SING), bad = cmr_slot_sum(nslots, nwg_n, Q_BAD);
  if (sing > 0.0 || bad > 0.0 || !isfinite(cost)) { st->code = 2; st->stop = 1; return; }   // the poses stay those step k - 1 started from
  double mw = 0.0, mv = 0.0;
  for (int s = 0; s < nwg_n; ++s) {
    mw = fmax(mw, nslots[(int64_t)s * PG_NS + Q_MAXW]);
    mv = fmax(mv, nslots[(int64_t)s * PG_NS + Q_MAXV]);
  }
  trace[5 * (int64_t)(k - 1) + 3] = mw;
  trace[5 * (int64_t)(k - 1) + 4] = mv;
  // A step within the tolerances stands and ends the loop, whatever the two costs: it changes the cost by less than the cost's rounding,
  // and comparing them would let that rounding decide which of two poses a tolerance apart is returned.
  const bool small = mw <= tol_rot && mv <= tol_trans;
  if (!small && !(cost < st->cost_prev)) { st->code = 0; st->stop = 1; return; }              // undone: the buffers do not flip
  st->which ^= 1;
  st->cost_prev = cost;
  if (small) { st->code = 0; st->stop = 1; return; }
  if (k < iters) trace[5 * (int64_t)k] = cost;
}

// One node per lane: M_n = sum A_e + damping I and g_n = sum +- b_e over its incidence in incidence order; M_n^-1 as its 21 upper entries,
// column j from cmr_pnp_chol6's solve against the unit vector e_j (rows i <= j kept, so the inverse is symmetric by construction);
// x = 0, r = -g, z = M^-1 r.  A fixed node's rows are 0.  A free node whose block does not factor is counted, and its inverse is 0.
__global__ __launch_bounds__(PG_T) void pg_blocks_kernel(PgState* __restrict__ st, int64_t F, int64_t E, const int32_t* __restrict__ edges,
                                                         const int32_t* __restrict__ inc_off, const int32_t* __restrict__ inc_edge,
                                                         const uint8_t* __restrict__ fixed, const double* __restrict__ A,
                                                         const double* __restrict__ b, double damping, double* __restrict__ Minv,
                                                         double* __restrict__ x, double* __restrict__ r, double* __restrict__ z,
                                                         double* __restrict__ nslots) {
  __shared__ double sm[PG_T / 64];
  if (st->stop) return;
  const int64_t n = (int64_t)blockIdx.x * PG_T + threadIdx.x;
  const bool live = n < F, free_node = live && !fixed[n];
  double M[21] = {}, g[6] = {}, Mi[21] = {};
  bool sing = false;
  if (free_node) {
    int64_t lo = inc_off[n], hi = inc_off[n + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > 2 * E ? 2 * E : hi;
    for (int64_t q = lo; q < hi; ++q) {
      const int64_t e = inc_edge[q];
      if (e < 0 || e >= E) continue;
      const int64_t i = edges[2 * e], j = edges[2 * e + 1];
      if (i == j || (n != i && n != j)) continue;
      const double sgn = n == i ? 1.0 : -1.0;
#pragma unroll
      for (int t = 0; t < 21; ++t) M[t] += A[21 * e + t];
#pragma unroll
      for (int t = 0; t < 6; ++t) g[t] += sgn * b[6 * e + t];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) M[pg_up(i, i)] += damping;
    for (int j = 0; j < 6; ++j) {
      double unit[6] = {}, col[6] = {};
      unit[j] = 1.0;
      if (!cmr_pnp_chol6<true>(M, unit, col)) sing = true;
      for (int i = 0; i <= j; ++i) Mi[pg_up(i, j)] = col[i];
    }
    bool ok = !sing;
    for (int t = 0; t < 21; ++t) ok = ok && isfinite(Mi[t]);
    for (int t = 0; t < 6; ++t) ok = ok && isfinite(g[t]);
    if (!ok) {
      sing = true;
      for (int t = 0; t < 21; ++t) Mi[t] = 0.0;
      for (int t = 0; t < 6; ++t) g[t] = 0.0;
    }
  }
  double rr[6], zz[6], rz = 0.0;
#pragma unroll
  for (int t = 0; t < 6; ++t) rr[t] = -g[t];
  pg_symv(Mi, rr, zz);
#pragma unroll
  for (int t = 0; t < 6; ++t) rz += rr[t] * zz[t];
  if (live) {
#pragma unroll
    for (int t = 0; t < 21; ++t) Minv[21 * n + t] = Mi[t];
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      x[6 * n + t] = 0.0;
      r[6 * n + t] = rr[t];
      z[6 * n + t] = zz[t];
    }
  }
  const double rz_wg = pg_block_sum(rz, sm), sing_wg = pg_block_sum(sing ? 1.0 : 0.0, sm);
  if (threadIdx.x == 0) {
    double* s = nslots + (int64_t)blockIdx.x * PG_NS;
    s[Q_RZ] = rz_wg;
    s[Q_RZ0] = rz_wg;
    s[Q_SING] = sing_wg;
    if (blockIdx.x == 0) st->done_a = st->used_a = st->done_b = st->used_b = 0;
  }
}

// CG iteration c, first half.  p_m = z_m + beta p_m(old) for the lane's node and, again, for every neighbour it meets (six multiply-adds
// each instead of a launch of its own); q_n = sum over the incidence, in incidence order, of +- A_e (p_i - p_j), then + damping p_n.
__global__ __launch_bounds__(PG_T) void pg_apply_kernel(PgState* __restrict__ st, int c, int nwg, int64_t F, int64_t E,
                                                        const int32_t* __restrict__ edges, const int32_t* __restrict__ inc_off,
                                                        const int32_t* __restrict__ inc_edge, const uint8_t* __restrict__ fixed,
                                                        const double* __restrict__ A, double damping, double cg_tol2,
                                                        const double* __restrict__ z, double* __restrict__ pbuf, double* __restrict__ qv,
                                                        double* __restrict__ nslots) {
  __shared__ double sm[PG_T / 64];
  if (st->stop || st->done_b) return;
  const double rz = cmr_slot_sum(nslots, nwg, Q_RZ + (c & 1)), rz0 = cmr_slot_sum(nslots, nwg, Q_RZ0);
  if (rz <= cg_tol2 * rz0) {
    if (blockIdx.x == 0 && threadIdx.x == 0) { st->used_a = c; st->done_a = 1; }
    return;
  }
  const double beta = c > 0 ? rz / cmr_slot_sum(nslots, nwg, Q_RZ + ((c + 1) & 1)) : 0.0;
  const double* __restrict__ pold = pbuf + (int64_t)((c + 1) & 1) * 6 * F;
  double* __restrict__ pnew = pbuf + (int64_t)(c & 1) * 6 * F;
  const int64_t n = (int64_t)blockIdx.x * PG_T + threadIdx.x;
  const bool live = n < F, free_node = live && !fixed[n];
  double pn[6] = {}, qn[6] = {};
  if (free_node) {
#pragma unroll
    for (int t = 0; t < 6; ++t) pn[t] = c > 0 ? z[6 * n + t] + beta * pold[6 * n + t] : z[6 * n + t];
    int64_t lo = inc_off[n], hi = inc_off[n + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > 2 * E ? 2 * E : hi;
    for (int64_t q = lo; q < hi; ++q) {
      const int64_t e = inc_edge[q];
      if (e < 0 || e >= E) continue;
      const int64_t i = edges[2 * e], j = edges[2 * e + 1];
      if (i == j || (n != i && n != j)) continue;
      const int64_t m = n == i ? j : i;
      double d[6] = {};
      if (m >= 0 && m < F && !fixed[m]) {
#pragma unroll
        for (int t = 0; t < 6; ++t) d[t] = c > 0 ? z[6 * m + t] + beta * pold[6 * m + t] : z[6 * m + t];
      }
      const double sgn = n == i ? 1.0 : -1.0;                    // d = p_i - p_j, and the term +- A_e d
#pragma unroll
      for (int t = 0; t < 6; ++t) d[t] = n == i ? pn[t] - d[t] : d[t] - pn[t];
      double Ae[21], Ad[6];
#pragma unroll
      for (int t = 0; t < 21; ++t) Ae[t] = A[21 * e + t];
      pg_symv(Ae, d, Ad);
#pragma unroll
      for (int t = 0; t < 6; ++t) qn[t] += sgn * Ad[t];
    }
#pragma unroll
    for (int t = 0; t < 6; ++t) qn[t] += damping * pn[t];
  }
  double pq = 0.0;
#pragma unroll
  for (int t = 0; t < 6; ++t) pq += pn[t] * qn[t];
  if (live) {
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      pnew[6 * n + t] = pn[t];
      qv[6 * n + t] = qn[t];
    }
  }
  const double pq_wg = pg_block_sum(pq, sm);
  if (threadIdx.x == 0) nslots[(int64_t)blockIdx.x * PG_NS + Q_PQ] = pq_wg;
}

// CG iteration c, second half: alpha = r.z / p.q, x += alpha p, r -= alpha q, z = M^-1 r, the next r.z.  p.q that is not positive and
// finite ends CG at x as it stands (H is not positive definite along p, or a value is not finite).
__global__ __launch_bounds__(PG_T) void pg_update_kernel(PgState* __restrict__ st, int c, int nwg, int64_t F, const uint8_t* __restrict__ fixed,
                                                         const double* __restrict__ Minv, const double* __restrict__ pbuf,
                                                         const double* __restrict__ qv, double* __restrict__ x, double* __restrict__ r,
                                                         double* __restrict__ z, double* __restrict__ nslots) {
  __shared__ double sm[PG_T / 64];
  if (st->stop) return;
  const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
  if (st->done_a) {
    if (writer && !st->done_b) { st->used_b = st->used_a; st->done_b = 1; }
    return;
  }
  const double pq = cmr_slot_sum(nslots, nwg, Q_PQ), rz = cmr_slot_sum(nslots, nwg, Q_RZ + (c & 1));
  if (!(pq > 0.0 && isfinite(pq) && isfinite(rz))) {
    if (writer && !st->done_b) { st->used_b = c; st->done_b = 1; }      // done_b is read by this thread alone among pg_update's
    return;
  }
  const double alpha = rz / pq;
  const double* __restrict__ p = pbuf + (int64_t)(c & 1) * 6 * F;
  const int64_t n = (int64_t)blockIdx.x * PG_T + threadIdx.x;
  double rz_new = 0.0;
  if (n < F && !fixed[n]) {
    double Mi[21], rr[6], zz[6];
#pragma unroll
    for (int t = 0; t < 21; ++t) Mi[t] = Minv[21 * n + t];
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      x[6 * n + t] += alpha * p[6 * n + t];
      rr[t] = r[6 * n + t] - alpha * qv[6 * n + t];
    }
    pg_symv(Mi, rr, zz);
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      r[6 * n + t] = rr[t];
      z[6 * n + t] = zz[t];
      rz_new += rr[t] * zz[t];
    }
  }
  const double rz_wg = pg_block_sum(rz_new, sm);
  if (threadIdx.x == 0) nslots[(int64_t)blockIdx.x * PG_NS + Q_RZ + ((c + 1) & 1)] = rz_wg;
}

// Step k: the candidate poses into the other buffer, the workgroup's largest |dw| and |dv| and its count of updates that are not finite;
// the CG part of trace row k.
__global__ __launch_bounds__(PG_T) void pg_step_kernel(PgState* __restrict__ st, int k, int cg_iters, int nwg, int64_t F,
                                                       const uint8_t* __restrict__ fixed, const double* __restrict__ x, double* __restrict__ buf,
                                                       double* __restrict__ nslots, double* __restrict__ trace) {
  __shared__ double sm[PG_T / 64];
  if (st->stop) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const int used = st->done_b ? st->used_b : cg_iters;
    const double rz = cmr_slot_sum(nslots, nwg, Q_RZ + (used & 1)), rz0 = cmr_slot_sum(nslots, nwg, Q_RZ0);
    trace[5 * (int64_t)k + 1] = (double)used;
    trace[5 * (int64_t)k + 2] = rz0 > 0.0 ? sqrt(rz / rz0) : 0.0;
    st->executed = k + 1;
  }
  const double* __restrict__ cur = buf + (int64_t)st->which * F * 12;
  double* __restrict__ cand = buf + (int64_t)(st->which ^ 1) * F * 12;
  const int64_t n = (int64_t)blockIdx.x * PG_T + threadIdx.x;
  double dw = 0.0, dv = 0.0, bad = 0.0;
  if (n < F) {
    double c12[12], nw[12];
#pragma unroll
    for (int t = 0; t < 12; ++t) c12[t] = cur[12 * n + t];
    if (!fixed[n]) {
      double xi[6];
#pragma unroll
      for (int t = 0; t < 6; ++t) xi[t] = x[6 * n + t];
      if (!cmr_pose_left_update(c12, xi, nw)) bad = 1.0;
      dw = sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]);
      dv = sqrt(xi[3] * xi[3] + xi[4] * xi[4] + xi[5] * xi[5]);
      if (!(isfinite(dw) && isfinite(dv))) { bad = 1.0; dw = dv = 0.0; }
    } else {
#pragma unroll
      for (int t = 0; t < 12; ++t) nw[t] = c12[t];
    }
#pragma unroll
    for (int t = 0; t < 12; ++t) cand[12 * n + t] = nw[t];
  }
  const double mw = pg_block_max(dw, sm), mv = pg_block_max(dv, sm), bad_wg = pg_block_sum(bad, sm);
  if (threadIdx.x == 0) {
    double* s = nslots + (int64_t)blockIdx.x * PG_NS;
    s[Q_MAXW] = mw;
    s[Q_MAXV] = mv;
    s[Q_BAD] = bad_wg;
  }
}

__global__ __launch_bounds__(PG_T) void pg_final_kernel(const PgState* __restrict__ st, int64_t F, const double* __restrict__ buf,
                                                        double* __restrict__ poses, double* __restrict__ cost, int32_t* __restrict__ status) {
  const double* __restrict__ cur = buf + (int64_t)st->which * F * 12;
  const int64_t n = (int64_t)blockIdx.x * PG_T + threadIdx.x;
  if (n < F) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) poses[16 * n + 4 * i + j] = cur[12 * n + 3 * i + j];
      poses[16 * n + 4 * i + 3] = cur[12 * n + 9 + i];
    }
    poses[16 * n + 12] = poses[16 * n + 13] = poses[16 * n + 14] = 0.0;
    poses[16 * n + 15] = 1.0;
  }
  if (n == 0) {
    cost[0] = st->cost_prev;
    status[0] = st->code;
    status[1] = st->executed;
    status[2] = st->wide;
  }
}

inline int64_t pg_wgs(int64_t n) { return (n + PG_T - 1) / PG_T; }
// the sizes a call takes: the node and edge vectors are indexed with 32-bit products in the wrapper's checks and must stay below 2^31
inline bool pg_sizes_ok(int64_t F, int64_t E) { return F > 0 && E > 0 && 6 * F < ((int64_t)1 << 31) && 28 * E < ((int64_t)1 << 31); }

struct PgWs { int64_t state, eslots, wslots, nslots, buf, A, b, Minv, x, r, z, p, q, total; };
inline PgWs pg_layout(int64_t F, int64_t E) {
  PgWs L;
  int64_t o = 0;
  auto take = [&](int64_t bytes) { const int64_t at = o; o += cmr_up16(bytes); return at; };
  L.state = take(sizeof(PgState));
  L.eslots = take(pg_wgs(E) * PG_NS * 8);
  L.wslots = take(pg_wgs(E) * 4);
  L.nslots = take(pg_wgs(F) * PG_NS * 8);
  L.buf = take(2 * F * 12 * 8);
  L.A = take(E * 21 * 8);
  L.b = take(E * 6 * 8);
  L.Minv = take(F * 21 * 8);
  L.x = take(F * 6 * 8);
  L.r = take(F * 6 * 8);
  L.z = take(F * 6 * 8);
  L.p = take(2 * F * 6 * 8);
  L.q = take(F * 6 * 8);
  L.total = o;
  return L;
}

}  // namespace

extern "C" int64_t cmr_pose_graph_linearize_workspace_bytes(int64_t E) {
  return E > 0 ? cmr_up16(pg_wgs(E) * PG_NS * 8) + cmr_up16(pg_wgs(E) * 4) : 0;
}

extern "C" int cmr_pose_graph_linearize_f64(const double* poses, int64_t F, const int32_t* edges, const double* meas, const double* weights,
                                            int64_t E, double huber, double* r, double* chi, double* scale, double* A, double* b, double* cost,
                                            int32_t* wide, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  CMR_REQUIRE(poses && edges && meas && weights && r && chi && scale && A && b && cost && wide && workspace && pg_sizes_ok(F, E));
  CMR_REQUIRE(huber >= 0.0 && std::isfinite(huber) && cmr_aligned16(workspace) && workspace_bytes >= cmr_pose_graph_linearize_workspace_bytes(E));
  const int nwg = (int)pg_wgs(E);
  double* slots = (double*)workspace;
  int32_t* wslots = (int32_t*)((char*)workspace + cmr_up16((int64_t)nwg * PG_NS * 8));
  hipLaunchKernelGGL(pg_linearize_kernel<16>, dim3(nwg), dim3(PG_T), 0, stream, poses, (const PgState*)nullptr, 0, F, edges, meas, weights, E,
                     huber, r, chi, scale, A, b, slots, wslots);
  hipLaunchKernelGGL(pg_total_kernel, dim3(1), dim3(64), 0, stream, (const double*)slots, (const int32_t*)wslots, nwg, cost, wide);
  return cmr_launch_status();
}

extern "C" int64_t cmr_pose_graph_optimize_workspace_bytes(int64_t F, int64_t E) { return pg_sizes_ok(F, E) ? pg_layout(F, E).total : 0; }

extern "C" int cmr_pose_graph_optimize_f64(const double* poses_in, int64_t F, const int32_t* edges, const double* meas, const double* weights,
                                           int64_t E, const int32_t* inc_offsets, const int32_t* inc_edges, const uint8_t* fixed, double huber,
                                           int iters, int cg_iters, double cg_tol, double damping, double tol_rot, double tol_trans,
                                           double* poses, double* cost, double* trace, int32_t* status, void* workspace,
                                           int64_t workspace_bytes, hipStream_t stream) {
  CMR_REQUIRE(poses_in && edges && meas && weights && inc_offsets && inc_edges && fixed && poses && cost && status && workspace &&
              pg_sizes_ok(F, E));
  CMR_REQUIRE(huber >= 0.0 && std::isfinite(huber) && iters >= 0 && iters <= 100 && cg_iters >= 0 && cg_iters <= 4096 && (iters == 0 || trace) &&
              cg_tol >= 0.0 && std::isfinite(cg_tol) && damping >= 0.0 && std::isfinite(damping) && tol_rot >= 0.0 && std::isfinite(tol_rot) &&
              tol_trans >= 0.0 && std::isfinite(tol_trans));
  CMR_REQUIRE(cmr_aligned16(workspace) && workspace_bytes >= cmr_pose_graph_optimize_workspace_bytes(F, E));
  const PgWs L = pg_layout(F, E);
  char* w = (char*)workspace;
  PgState* st = (PgState*)(w + L.state);
  double *eslots = (double*)(w + L.eslots), *nslots = (double*)(w + L.nslots), *buf = (double*)(w + L.buf), *A = (double*)(w + L.A),
         *b = (double*)(w + L.b), *Minv = (double*)(w + L.Minv), *x = (double*)(w + L.x), *r = (double*)(w + L.r), *z = (double*)(w + L.z),
         *p = (double*)(w + L.p), *q = (double*)(w + L.q);
  int32_t* wslots = (int32_t*)(w + L.wslots);
  const int nwg_e = (int)pg_wgs(E), nwg_n = (int)pg_wgs(F);
  const int64_t init_lanes = F > (int64_t)iters * 5 ? F : (int64_t)iters * 5;
  hipLaunchKernelGGL(pg_init_kernel, dim3((unsigned)pg_wgs(init_lanes)), dim3(PG_T), 0, stream, poses_in, F, iters, st, buf, trace);
  for (int k = 0; k <= iters; ++k) {
    hipLaunchKernelGGL(pg_linearize_kernel<12>, dim3(nwg_e), dim3(PG_T), 0, stream, (const double*)buf, (const PgState*)st, k > 0 ? 1 : 0, F,
                       edges, meas, weights, E, huber, (double*)nullptr, (double*)nullptr, (double*)nullptr, A, b, eslots, wslots);
    hipLaunchKernelGGL(pg_begin_kernel, dim3(1), dim3(64), 0, stream, k, iters, nwg_e, nwg_n, tol_rot, tol_trans, st, (const double*)eslots,
                       (const int32_t*)wslots, (const double*)nslots, trace);
    if (k == iters) break;
    hipLaunchKernelGGL(pg_blocks_kernel, dim3(nwg_n), dim3(PG_T), 0, stream, st, F, E, edges, inc_offsets, inc_edges, fixed, (const double*)A,
                       (const double*)b, damping, Minv, x, r, z, nslots);
    for (int c = 0; c < cg_iters; ++c) {
      hipLaunchKernelGGL(pg_apply_kernel, dim3(nwg_n), dim3(PG_T), 0, stream, st, c, nwg_n, F, E, edges, inc_offsets, inc_edges, fixed,
                         (const double*)A, damping, cg_tol * cg_tol, (const double*)z, p, q, nslots);
      hipLaunchKernelGGL(pg_update_kernel, dim3(nwg_n), dim3(PG_T), 0, stream, st, c, nwg_n, F, fixed, (const double*)Minv, (const double*)p,
                         (const double*)q, x, r, z, nslots);
    }
    hipLaunchKernelGGL(pg_step_kernel, dim3(nwg_n), dim3(PG_T), 0, stream, st, k, cg_iters, nwg_n, F, fixed, (const double*)x, buf, nslots, trace);
  }
  hipLaunchKernelGGL(pg_final_kernel, dim3(nwg_n), dim3(PG_T), 0, stream, (const PgState*)st, F, (const double*)buf, poses, cost, status);
  return cmr_launch_status();
}
