// Newton mode (SGDNET_MODE_NEWTON): the binomial elastic-net path of one response by proximal Newton steps (IRLS).
//
// The problem is the one every mode fits (sgdnet_amd/kkt.py): features z_j = (x_j - m_j) / s_j, u = (w, b),
//     F(u) = (1/n) sum_i [log(1 + e^eta_i) - y_i eta_i] + alpha/2 |w|^2 + beta |w|_1,     eta_i = b + z_i'w,
// b unpenalised (or frozen at the null model's value), alpha and beta the driver's (regularization_path).  m are the
// fixed, unweighted column means of cov_sum_kernel (0 where the fit centres nothing): the optimum does not depend on
// them, the conditioning of the quadratic model does.  One outer step from the iterate u0, warm-started lambda to lambda:
//
//   state      newton_state_kernel: eta_i, t_i = 1 / (1 + e^eta_i), v_i = t_i (1 - t_i), r_i = y_i - mu_i and the loss,
//              a thread per sample; exp / log are the plain-IEEE ones of include/sgdnet_detmath.h.  Deviations are
//              formed BEFORE they are multiplied: (x_ij - m_j) (w_j / s_j).  Dense x is read column-major; sparse x
//              is read from the sample-major copy of device_transpose, whose rows hold their columns in ascending
//              order: one walk over j = 0 .. p - 1 takes the stored value or 0 (no m'w subtracted from a sum afterwards).
//              newton_finish_kernel adds the workgroups' sums of loss, v and r in workgroup order.
//   moments    H = (1/n) sum_i v_i [x_i - m | 1][x_i - m | 1]',  q = (1/n) sum_i r_i [x_i - m | 1]   (f64; the 1/n and the
//              driver's s_j are applied when the inner solve loads them), as an upper triangle of (p + 2)^2: column p
//              is the ones, column p + 1 is q.
//              dense x   newton_dense_tile_kernel: cov_dense_tile_kernel with the rows of the second tile weighted at
//                        staging (v_i; the q column is staged as r_i); cov_reduce_kernel adds the chunks in chunk order.
//              sparse x  newton_sparse_pair_kernel: a workgroup owns a pair of columns, centred implicitly with weights:
//                          H_jk = sum_{J and K} v d_j d_k - m_k sum_{J \ K} v d_j - m_j sum_{K \ J} v d_k
//                                 + (V - sum_{J or K} v) m_j m_k,      d = stored value - mean,  V = sum_i v_i,
//                        the ones column  sum_J v d_j - m_j (V - sum_J v)  and q_j = sum_J r d_j - m_j (R - sum_J r),
//                        R = sum_i r_i; a column that stores every row leaves nothing outside it (an exact 0).
//   inner      newton_cd_kernel: ONE wavefront keeps H (packed triangle), u and g = H (u - u0) - q in LDS (newton.hpp:
//              the budget behind sgdnet_newton_max_features) and runs cyclic coordinate descent with the update rule
//              and the uniform-scalar style of cov_path_kernel; the last coordinate, the intercept, has no penalty
//              and no threshold.  A sweep ends with the reference's ConvergenceCheck over all of u.
//   accept     the state pass at the candidate gives its objective; the host halves a step after which it rose
//              (newton_blend_kernel) and evaluates again, at most kNewtonMaxHalvings times.  The accepted candidate's
//              state pass is the next step's: it costs no extra pass.
//
// The outer loop is the host's (newton_run): separate launches on one stream and one small record read back per state
// pass.  No floating-point atomic anywhere and every reduction in an order fixed by (n, p, nnz): the same input gives
// the same bits.
//
// Wide mode (wnewton_run, SGDNET_MODE_WNEWTON): beyond 198 features H does not fit one workgroup's LDS.  The loop, the state
// pass and the dense moments kernels are the ones above (row chunks by wide_layout.hpp's wide_row_chunks); then
// wide_scale_kernel writes H = M / n / (s s') to global memory as a full symmetric matrix with diag H and q, and
// newton_wide_cd_kernel keeps g, u, diag H and an ascending list of the coordinates that can move in LDS, sweeps that
// list, reads one column of H per move and lets a screen with the full gradient add coordinates (newton.hpp: the budget
// behind sgdnet_wnewton_max_features).  The scale kernel, the list compaction and the column move are wide_cd_device.hpp's,
// shared with covariance.hip.  Dense x only: the driver expands sparse x.
//
// Cross-validation (newton_cv_run, include/sgdnet_hip.h: sgdnet_cv_newton_*): all fold fits of all mixes advance in
// lock-step.  The rows are sorted by group once, so a training set is a range of rows or the complement of one; the
// newton_cv_* kernels are the kernels above with a job dimension, each job on its own rows, centres, scales and buffers;
// the host keeps newton_run's state machine once per job, sends one command per job and round and reads all records
// back in one copy.
//
// Wide cross-validation (wnewton_cv_run, include/sgdnet_hip.h: sgdnet_cv_wnewton_*): the same loop around the wide inner
// solve, dense x only.  The state, finish, dense tile and reduce kernels are the narrow CV's on the row chunks wnewton_run
// would choose for each job's rows; newton_cv_wide_scale_kernel, newton_cv_wide_cd_kernel and newton_cv_wide_blend_kernel are
// the wide kernels with a job dimension, every job with its own H, diag H and q in global memory (H depends on the iterate:
// nothing is pooled across jobs) and one workgroup -- one compute unit -- per job and round.
#define SGDNET_DET_MATH
#include <algorithm>
#include <utility>
#include <vector>

#include "common.hpp"
#include "device_math.hpp"
#include "moments_device.hpp"
#include "newton.hpp"
#include "newton_cv_device.hpp"
#include "setup_device.hpp"
#include "wide_cd_device.hpp"

namespace sgdnet {
namespace {

constexpr int kStateMaxBlocks = 1024;   // workgroups of the state pass: each leaves three sums

// a[j] = w_j / s_j (j < p), a[p] = b: the candidate as the state pass multiplies it.  Workgroup b leaves its sums of
// the loss, v and r in partial[3 b ..].
template <bool kSparse>
__global__ __launch_bounds__(kBlock) void newton_state_kernel(const double* __restrict__ x, const int64_t* __restrict__ sptr,
                                                               const int32_t* __restrict__ sidx, const double* __restrict__ y,
                                                               const double* __restrict__ mu, const double* __restrict__ a, int64_t n,
                                                               int p, int centre, double* __restrict__ v, double* __restrict__ r,
                                                               double* __restrict__ partial) {
  __shared__ double sh[kBlock];
  double loss = 0.0, vs = 0.0, rs = 0.0;
  const double b = a[p];
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    double eta = 0.0;
    if (kSparse) {
      int64_t q = sptr[i];
      const int64_t q1 = sptr[i + 1];
      if (centre) {
        for (int j = 0; j < p; ++j) {
          double d = -mu[j];
          if (q < q1 && sidx[q] == j) d = x[q++] - mu[j];
          eta += d * a[j];
        }
      } else {
        for (; q < q1; ++q) eta += x[q] * a[sidx[q]];
      }
    } else {
      for (int j = 0; j < p; ++j) eta += (x[i + (int64_t)j * n] - mu[j]) * a[j];
    }
    eta += b;
    const double yi = y[i];
    const double e = SGD_EXP(eta);
    const double t = 1.0 / (1.0 + e);
    const double vi = t * (1.0 - t), ri = t - (1.0 - yi);     // y - mu, mu = 1 - t (families.h: Gradient = 1 - y - t)
    v[i] = vi;
    r[i] = ri;
    loss += SGD_LOG(1.0 + e) - yi * eta;
    vs += vi;
    rs += ri;
  }
  loss = block_sum(loss, sh);
  vs = block_sum(vs, sh);
  rs = block_sum(rs, sh);
  if (threadIdx.x == 0) {
    partial[3 * blockIdx.x] = loss;
    partial[3 * blockIdx.x + 1] = vs;
    partial[3 * blockIdx.x + 2] = rs;
  }
}

// one workgroup: the sums of the state pass added in workgroup order; rec gets the mean loss, sums = (V, R)
__global__ __launch_bounds__(kBlock) void newton_finish_kernel(const double* __restrict__ partial, int blocks, int64_t n,
                                                                double* __restrict__ sums, double* __restrict__ rec) {
  __shared__ double sh[kBlock];
  double s[3] = {0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < blocks; b += kBlock)
    for (int c = 0; c < 3; ++c) s[c] += partial[3 * b + c];
  for (int c = 0; c < 3; ++c) s[c] = block_sum(s[c], sh);
  if (threadIdx.x == 0) {
    rec[kRecLoss] = s[0] / (double)n;
    sums[0] = s[1];
    sums[1] = s[2];
  }
}

// cov_dense_tile_kernel for the rows [x - mu | 1 | r] with the second tile's rows weighted: entry (a, b), a <= b, of the
// (p + 2)^2 matrix is sum_i A_ia B_ib with A = [x - mu | 1 | 0] and B = [v (x - mu) | v | r].
__global__ __launch_bounds__(kBlock) void newton_dense_tile_kernel(const double* __restrict__ x, const double* __restrict__ v,
                                                                    const double* __restrict__ r, const double* __restrict__ mu,
                                                                    int64_t n, int p, int64_t rows_per_chunk, double* __restrict__ part) {
  __shared__ double A[kTileCols][kTileRows + 1], B[kTileCols][kTileRows + 1];
  const int tid = threadIdx.x, ncols = p + 2;
  const int T = (ncols + kTileCols - 1) / kTileCols;
  int pair = blockIdx.x, tj = 0;
  while (pair >= T - tj) {
    pair -= T - tj;
    ++tj;
  }
  const int tk = tj + pair;
  const int ta = tid & (kTileCols - 1), tb = tid / kTileCols;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_chunk;
  const int64_t r1 = r0 + rows_per_chunk < n ? r0 + rows_per_chunk : n;
  auto dev = [&](int a, int64_t i) -> double {          // column a of [x - mu | 1], 0 outside it
    if (i >= r1 || a > p) return 0.0;
    return a < p ? x[i + (int64_t)a * n] - mu[a] : 1.0;
  };
  double acc = 0.0;
  for (int64_t base = r0; base < r1; base += kTileRows) {
    for (int e = tid; e < kTileCols * kTileRows; e += kBlock) {
      const int row = e & (kTileRows - 1), col = e / kTileRows;
      const int64_t i = base + row;
      const int b = tk * kTileCols + col;
      A[col][row] = dev(tj * kTileCols + col, i);
      B[col][row] = i >= r1 ? 0.0 : (b == p + 1 ? r[i] : v[i] * dev(b, i));
    }
    __syncthreads();
    for (int i = 0; i < kTileRows; ++i) acc += A[ta][i] * B[tb][i];
    __syncthreads();
  }
  part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kBlock + tid] = acc;
}

// blockIdx.x = column j < p, blockIdx.y = column k in [j, p + 1]; k == p is the ones, k == p + 1 is q.  sums = (V, R).
// The workgroup (0, p) also leaves the corner (ones, ones) = V and (0, p + 1) leaves q of the ones, R.
__global__ __launch_bounds__(kBlock) void newton_sparse_pair_kernel(const int32_t* __restrict__ colptr, const int32_t* __restrict__ rowidx,
                                                                     const double* __restrict__ val, const double* __restrict__ v,
                                                                     const double* __restrict__ r, const double* __restrict__ mu,
                                                                     const double* __restrict__ sums, int64_t n, int p,
                                                                     double* __restrict__ M) {
  __shared__ double sh[kBlock];
  const int j = blockIdx.x, k = blockIdx.y, nc = p + 2, tid = threadIdx.x;
  if (k < j) return;
  const int q0 = colptr[j], q1 = colptr[j + 1];
  const double mj = mu[j];
  const bool j_full = (int64_t)(q1 - q0) == n;
  if (k >= p) {                                  // against the ones (weights v) or q (weights r)
    const double* wt = k == p ? v : r;
    double a = 0.0, ws = 0.0;
    for (int q = q0 + tid; q < q1; q += kBlock) {
      const double wi = wt[rowidx[q]];
      a += wi * (val[q] - mj);
      ws += wi;
    }
    a = block_sum(a, sh);
    ws = block_sum(ws, sh);
    if (tid == 0) {
      const double total = sums[k - p];
      M[(size_t)j * nc + k] = a - mj * (j_full ? 0.0 : total - ws);
      if (j == 0) M[(size_t)p * nc + k] = total;
    }
    return;
  }
  const int s0 = colptr[k], s1 = colptr[k + 1];
  const double mk = mu[k];
  double both = 0.0, only_j = 0.0, only_k = 0.0, v_union = 0.0;
  for (int q = q0 + tid; q < q1; q += kBlock) {
    const int32_t row = rowidx[q];
    const double vi = v[row], d = val[q] - mj;
    v_union += vi;
    const int pos = j == k ? q : lower_bound_row(rowidx, s0, s1, row);
    if (pos < s1 && rowidx[pos] == row) both += vi * d * (val[pos] - mk);
    else only_j += vi * d;
  }
  if (j != k)
    for (int s = s0 + tid; s < s1; s += kBlock) {
      const int32_t row = rowidx[s];
      const int pos = lower_bound_row(rowidx, q0, q1, row);
      if (!(pos < q1 && rowidx[pos] == row)) {
        const double vi = v[row];
        only_k += vi * (val[s] - mk);
        v_union += vi;
      }
    }
  both = block_sum(both, sh);
  only_j = block_sum(only_j, sh);
  only_k = block_sum(only_k, sh);
  v_union = block_sum(v_union, sh);
  if (tid == 0) {
    const bool full = j_full || (int64_t)(s1 - s0) == n;
    const double in_neither = full ? 0.0 : sums[0] - v_union;
    M[(size_t)j * nc + k] = both - mk * only_j - mj * only_k + in_neither * mj * mk;
  }
}

// What a candidate un[0 .. P) leaves behind, by one wavefront: itself and its state-pass form a (w_j / s_j, b) in
// memory, and in the record its penalty terms |w|^2 / 2 and |w|_1, its distance from the iterate max|un - u_cur| and
// its size max|un|.  Lane l takes the coordinates l, l + 64, ... in order; the lanes are joined by a butterfly.
template <class UP>
__device__ __forceinline__ void publish_candidate(UP un, const double* __restrict__ u_cur, const double* __restrict__ scale, int p,
                                                  double* __restrict__ u_cand, double* __restrict__ a_cand, double* __restrict__ rec) {
  const int lane = threadIdx.x;
  double sq = 0.0, ab = 0.0, ch = 0.0, sz = 0.0;
  for (int k = lane; k <= p; k += 64) {
    const double uk = un[k];
    ch = fmax(ch, fabs(uk - u_cur[k]));
    sz = fmax(sz, fabs(uk));
    if (k < p) {
      sq += uk * uk;
      ab += fabs(uk);
    }
    u_cand[k] = uk;
    a_cand[k] = k < p ? uk / scale[k] : uk;
  }
  sq = wave_sum(sq);
  ab = wave_sum(ab);
  ch = wave_max(ch);
  sz = wave_max(sz);
  if (lane == 0) {
    rec[kRecHalfSq] = 0.5 * sq;
    rec[kRecAbs] = ab;
    rec[kRecChange] = ch;
    rec[kRecSize] = sz;
  }
}

// u_cand <- u_cur + t (u_cand - u_cur)   (t = 1: the candidate as it is; the path's start is published this way)
__global__ __launch_bounds__(64) void newton_blend_kernel(const double* __restrict__ u_cur, const double* __restrict__ scale, int p,
                                                           double t, double* __restrict__ u_cand, double* __restrict__ a_cand,
                                                           double* __restrict__ rec) {
  __shared__ double un[kNewtonMaxFeatures + 1];
  for (int k = threadIdx.x; k <= p; k += 64) un[k] = t == 1.0 ? u_cand[k] : u_cur[k] + t * (u_cand[k] - u_cur[k]);
  __syncthreads();
  publish_candidate(un, u_cur, scale, p, u_cand, a_cand, rec);
}

// One wavefront, one inner solve.  Every lane computes the sweep's scalars (the new coordinate, the sweep's max|du| and
// max|u|) from the same LDS words, so branches on them are uniform and nothing has to be broadcast (cov_path_kernel).
// M: the (p + 2)^2 moments (upper triangle), dn = n; the quadratic model about u_cur is
//   (u - u_cur)'H (u - u_cur) / 2 - q'(u - u_cur) + al/2 |w|^2 + be |w|_1,     its smooth gradient g = H (u - u_cur) - q.
// (the body of newton_cd_kernel and of newton_cv_cd_kernel, which runs it once per job; lds: the workgroup's whole LDS)
__device__ __forceinline__ void newton_cd_solve(double* lds, const double* __restrict__ M, const double* __restrict__ scale, int p, double dn,
                                                const double* __restrict__ u_cur, double al, double be, int ridge, int fit_intercept,
                                                unsigned max_sweeps, double tol, double* __restrict__ u_cand, double* __restrict__ a_cand,
                                                double* __restrict__ rec) {
  const int lane = threadIdx.x, P = p + 1, nc = p + 2;
  double* H = lds;
  double* u = H + P * (P + 1) / 2;
  double* g = u + P;
  for (int k = 0; k < P; ++k) {
    const double sk = k < p ? scale[k] : 1.0;
    for (int j = lane; j <= k; j += 64) H[tri(j, k)] = M[(size_t)j * nc + k] / dn / ((j < p ? scale[j] : 1.0) * sk);
  }
  for (int k = lane; k < P; k += 64) {
    g[k] = -(M[(size_t)k * nc + p + 1] / dn / (k < p ? scale[k] : 1.0));
    u[k] = u_cur[k];
  }
  __syncthreads();
  const int n_coord = fit_intercept ? P : p;     // (the frozen intercept is never visited: it stays at u_cur[p])
  unsigned sweeps = 0;
  bool converged = false, negligible = false;
  while (sweeps < max_sweeps && !converged) {
    double max_change = 0.0, max_size = 0.0, max_eta_sq = 0.0;
    for (int j = 0; j < n_coord; ++j) {
      const bool penalised = j < p;
      const double uj = u[j], hjj = H[tri(j, j)];
      const double z = hjj * uj - g[j], denom = penalised ? hjj + al : hjj;
      double nu = z;
      if (penalised && !ridge) nu = z > be ? z - be : (z < -be ? z + be : 0.0);
      // a constant column without an l2 term: H_jj = q_j = 0; every weight underflowed: the intercept stays
      nu = denom > 0.0 ? nu / denom : (penalised ? 0.0 : uj);
      const double d = nu - uj;
      max_change = fmax(max_change, fabs(d));
      max_size = fmax(max_size, fabs(nu));
      max_eta_sq = fmax(max_eta_sq, nu * nu * hjj);
      if (d != 0.0) {
        __syncthreads();                         // every lane has read u[j] and g[j]
        if (lane == 0) u[j] = nu;
        for (int k = lane; k < P; k += 64) g[k] += H[k <= j ? tri(k, j) : tri(j, k)] * d;
        __syncthreads();
      }
    }
    ++sweeps;
    const bool all_zero = max_size == 0.0 && max_change == 0.0;
    const bool no_change = max_size != 0.0 && max_change / max_size <= tol;
    negligible = max_eta_sq <= kNewtonNegligible * kNewtonNegligible;      // zero to rounding (newton.hpp)
    converged = all_zero || no_change || negligible;
  }
  __syncthreads();
  publish_candidate(u, u_cur, scale, p, u_cand, a_cand, rec);
  if (lane == 0) {
    rec[kRecSweeps] = (double)sweeps;
    rec[kRecInnerConverged] = converged ? 1.0 : 0.0;
    rec[kRecNegligible] = negligible ? 1.0 : 0.0;
  }
}

__global__ __launch_bounds__(64) void newton_cd_kernel(const double* __restrict__ M, const double* __restrict__ scale, int p, double dn,
                                                        const double* __restrict__ u_cur, double al, double be, int ridge,
                                                        int fit_intercept, unsigned max_sweeps, double tol, double* __restrict__ u_cand,
                                                        double* __restrict__ a_cand, double* __restrict__ rec) {
  __shared__ double lds[newton_state_doubles(kNewtonMaxFeatures)];
  newton_cd_solve(lds, M, scale, p, dn, u_cur, al, be, ridge, fit_intercept, max_sweeps, tol, u_cand, a_cand, rec);
}

// ---- wide Newton mode (SGDNET_MODE_WNEWTON, wnewton_run): H in global memory, only what can move is touched ----

// newton_blend_kernel without an array of kNewtonMaxFeatures + 1 doubles: publish_candidate reads every coordinate once,
// by the lane that then writes it, so the blend is formed where it is read.
struct BlendedCandidate {
  const double* u_cur;
  const double* u_cand;
  double t;
  __device__ __forceinline__ double operator[](int k) const { return t == 1.0 ? u_cand[k] : u_cur[k] + t * (u_cand[k] - u_cur[k]); }
};

__global__ __launch_bounds__(64) void newton_wide_blend_kernel(const double* u_cur, const double* __restrict__ scale, int p, double t,
                                                                double* u_cand, double* __restrict__ a_cand, double* __restrict__ rec) {
  publish_candidate(BlendedCandidate{u_cur, u_cand, t}, u_cur, scale, p, u_cand, a_cand, rec);
}

// The coordinate update of newton_cd_solve, for the screen (u_j = 0) and for the sweep: from H_jj, u_j and g_j to the new
// u_j.  Every caller passes the same words through the same operations, so every lane holds the same bits.
__device__ __forceinline__ double newton_coord_new_u(double hjj, double uj, double gj, double al, double be, int ridge, bool penalised) {
  const double z = hjj * uj - gj, denom = penalised ? hjj + al : hjj;
  double nu = z;
  if (penalised && !ridge) nu = z > be ? z - be : (z < -be ? z + be : 0.0);
  // a constant column without an l2 term: H_jj = q_j = 0; every weight underflowed: the intercept stays
  return denom > 0.0 ? nu / denom : (penalised ? 0.0 : uj);
}

// One workgroup of kWidth lanes, one inner solve, H (leading dimension ld, a multiple of 16) read from global memory.
// LDS (newton.hpp: wnewton_state_bytes): g | u | diag H | the list | the list's bits | the compaction's counts.
//   start    u = u_cur, so g = H (u - u_cur) - q = -q exactly: no pass over H.  The list is {j < p : u_j != 0} and the
//            intercept coordinate p when it is fitted (unpenalised, without threshold; frozen: never visited).
//   screen   every j < p outside the list: the coordinate update from u_j = 0; those that would move join.  The list is
//            compacted again from its bits (wide_cd_device.hpp: wide_compact, cov_wide_path_kernel's too)
//   sweep    newton_cd_solve's coordinate update over the list: every lane computes the scalars from the same LDS words
//            (uniform branches); a coordinate that stays costs no global read and no barrier; one that moves by d does
//            g[k] += H[k, j] d for ALL k < P, 16 bytes a lane, so g stays the full gradient and the screen needs no
//            pass over H.  The sweeps end as newton_cd_solve's do; then the screen runs again, and the solve is done when
//            it adds nothing.
// max_sweeps bounds the list sweeps of the solve.  g[k] is updated by one lane from the same words in the same order
// whatever kWidth is, and the candidate is published by the first wavefront alone: both widths give the same bits.
// (the body of newton_wide_cd_kernel and of newton_cv_wide_cd_kernel, which runs it once per job; lds: the workgroup's
// kWnewtonLdsBytes, aligned to 16)
template <int kWidth>
__device__ __forceinline__ void newton_wide_cd_solve(unsigned char* lds, const double* __restrict__ H, const double* __restrict__ Hd,
                                                     const double* __restrict__ q, const double* __restrict__ scale, int p, int ld,
                                                     const double* __restrict__ u_cur, double al, double be, int ridge, int fit_intercept,
                                                     unsigned max_sweeps, double tol, double* __restrict__ u_cand,
                                                     double* __restrict__ a_cand, double* __restrict__ rec) {
  const int lane = threadIdx.x, wave = lane >> 6, P = p + 1;
  double* g = reinterpret_cast<double*>(lds);
  double* u = g + P;
  double* hd = u + P;
  int32_t* list = reinterpret_cast<int32_t*>(hd + P);
  uint32_t* bits = reinterpret_cast<uint32_t*>(list + P);
  int32_t* counts = reinterpret_cast<int32_t*>(bits + (P + 31) / 32);
  for (int k = lane; k < P; k += kWidth) {
    g[k] = -q[k];
    u[k] = u_cur[k];
    hd[k] = Hd[k];
  }
  __syncthreads();

  // The list from one flag per coordinate (wide_cd_device.hpp: wide_compact).  screen: the flag is "in the list already,
  // or would move from 0"; else: the start's.  Coordinate p is in iff the intercept is fitted.  (One functor with a
  // run-time `screen` and its own bounds, not one per call site: in this shape the kernel compiles to the instructions
  // it had with its own copy of the compaction.)
  auto compact = [&](bool screen) -> int {
    return wide_compact<kWidth>(P, list, bits, counts, [&](int j) -> bool {
      bool in = false;
      if (j < p) {
        if (screen) {
          in = (bits[j >> 5] >> (j & 31)) & 1u;
          if (!in) in = newton_coord_new_u(hd[j], 0.0, g[j], al, be, ridge, true) != 0.0;
        } else {
          in = u[j] != 0.0;
        }
      } else if (j == p) {
        in = fit_intercept != 0;
      }
      return in;
    });
  };

  int n_list = compact(false);
  unsigned sweeps = 0;
  bool converged = false, negligible = false;
  for (int screens = 0;; ++screens) {
    const int n_new = compact(true);
    if (screens > 0 && n_new == n_list) {        // the list had converged and nothing outside it moves
      converged = true;
      break;
    }
    n_list = n_new;
    bool met = false;
    while (sweeps < max_sweeps && !met) {
      double max_change = 0.0, max_size = 0.0, max_eta_sq = 0.0;
      for (int i = 0; i < n_list; ++i) {
        const int j = list[i];
        const double uj = u[j], hjj = hd[j];
        const double nu = newton_coord_new_u(hjj, uj, g[j], al, be, ridge, j < p);
        const double d = nu - uj;
        max_change = fmax(max_change, fabs(d));
        max_size = fmax(max_size, fabs(nu));
        max_eta_sq = fmax(max_eta_sq, nu * nu * hjj);
        if (d != 0.0) {
          __syncthreads();                         // every lane has read u[j] and g[j]
          if (lane == 0) u[j] = nu;
          wide_column_move<kWidth>(g, H + (size_t)ld * j, P, d);
          __syncthreads();
        }
      }
      ++sweeps;
      const bool all_zero = max_size == 0.0 && max_change == 0.0;
      const bool no_change = max_size != 0.0 && max_change / max_size <= tol;
      negligible = max_eta_sq <= kNewtonNegligible * kNewtonNegligible;      // zero to rounding (newton.hpp)
      met = all_zero || no_change || negligible;
    }
    if (!met) break;                               // max_sweeps: the next outer step goes on from here
  }
  __syncthreads();
  if (wave == 0) {
    publish_candidate(u, u_cur, scale, p, u_cand, a_cand, rec);
    if (lane == 0) {
      rec[kRecSweeps] = (double)sweeps;
      rec[kRecInnerConverged] = converged ? 1.0 : 0.0;
      rec[kRecNegligible] = negligible ? 1.0 : 0.0;
    }
  }
}

template <int kWidth>
__global__ __launch_bounds__(kWidth) void newton_wide_cd_kernel(const double* __restrict__ H, const double* __restrict__ Hd,
                                                                 const double* __restrict__ q, const double* __restrict__ scale, int p, int ld,
                                                                 const double* __restrict__ u_cur, double al, double be, int ridge,
                                                                 int fit_intercept, unsigned max_sweeps, double tol,
                                                                 double* __restrict__ u_cand, double* __restrict__ a_cand,
                                                                 double* __restrict__ rec) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[kWnewtonLdsBytes];
  newton_wide_cd_solve<kWidth>(lds, H, Hd, q, scale, p, ld, u_cur, al, be, ridge, fit_intercept, max_sweeps, tol, u_cand, a_cand, rec);
}

// The wide inner solve's workgroup.  Both instances give the same bits; profiles/wnewton_path.txt has the inner solves'
// time per 100-lambda path at p = 198, 1000, 2000 and 4000:
//   lanes      p = 198     1000     2000     4000
//   256        31.6 ms   279 ms   597 ms   970 ms
//   1024       41.0 ms   267 ms   288 ms   426 ms
// A column of 199 doubles is less than one stride of 256 lanes, and twelve more wavefronts only wait at the barriers; at
// 1000 the two are within 4 %, from 2000 on sixteen wavefronts halve the solve.  So cov_wide_path_kernel's rule
// (wide_layout.hpp: wide_cd_width) stands here: 256 lanes up to 512 features, 1024 beyond.  That kernel's look-ahead
// variant is not built: at p = 4000, where it gained a quarter there, the inner solve is 41 % of a fit that the moments
// and the state pass make 3.8 times slower than auto.

// ---- cross-validation (newton_cv_run): the kernels above with a job dimension ----
// A job is one (mix, training set), its command, its rows (cv_row) and its record as newton_cv_device.hpp has them.  Every
// job has its own a, v, r, sums, moments, record, two iterates and slice of U; its centres and scales are its training
// set's; its grids (state workgroups, row chunks) are those newton_run would choose for n_t rows, so its arithmetic is
// the same whichever other jobs share the launch.

// newton_state_kernel for the job blockIdx.y; workgroup b of the job leaves its sums in partial[job][3 b ..]
template <bool kSparse>
__global__ __launch_bounds__(kBlock) void newton_cv_state_kernel(const CvCmd* __restrict__ cmd, const CvJob* __restrict__ jobs,
                                                                  const double* __restrict__ x, const int64_t* __restrict__ sptr,
                                                                  const int32_t* __restrict__ sidx, const double* __restrict__ y,
                                                                  const double* __restrict__ mu_all, const double* __restrict__ a_all,
                                                                  int64_t n, int p, int centre, double* __restrict__ v_all,
                                                                  double* __restrict__ r_all, double* __restrict__ partial_all) {
  __shared__ double sh[kBlock];
  const int job = blockIdx.y;
  if (cmd[job].action == kCvIdle) return;
  const CvJob J = jobs[job];
  if ((int)blockIdx.x >= J.state_blocks) return;
  const double* __restrict__ mu = mu_all + (size_t)J.set * (size_t)p;
  const double* __restrict__ a = a_all + (size_t)job * (size_t)(p + 1);
  double* __restrict__ v = v_all + (size_t)job * (size_t)n;
  double* __restrict__ r = r_all + (size_t)job * (size_t)n;
  double* __restrict__ partial = partial_all + (size_t)job * 3 * kStateMaxBlocks;
  double loss = 0.0, vs = 0.0, rs = 0.0;
  const double b = a[p];
  for (int64_t li = (int64_t)blockIdx.x * kBlock + threadIdx.x; li < J.n_t; li += (int64_t)J.state_blocks * kBlock) {
    const int64_t i = cv_row(J, li);
    double eta = 0.0;
    if (kSparse) {
      int64_t q = sptr[i];
      const int64_t q1 = sptr[i + 1];
      if (centre) {
        for (int j = 0; j < p; ++j) {
          double d = -mu[j];
          if (q < q1 && sidx[q] == j) d = x[q++] - mu[j];
          eta += d * a[j];
        }
      } else {
        for (; q < q1; ++q) eta += x[q] * a[sidx[q]];
      }
    } else {
      for (int j = 0; j < p; ++j) eta += (x[i + (int64_t)j * n] - mu[j]) * a[j];
    }
    eta += b;
    const double yi = y[i];
    const double e = SGD_EXP(eta);
    const double t = 1.0 / (1.0 + e);
    const double vi = t * (1.0 - t), ri = t - (1.0 - yi);
    v[i] = vi;
    r[i] = ri;
    loss += SGD_LOG(1.0 + e) - yi * eta;
    vs += vi;
    rs += ri;
  }
  loss = block_sum(loss, sh);
  vs = block_sum(vs, sh);
  rs = block_sum(rs, sh);
  if (threadIdx.x == 0) {
    partial[3 * blockIdx.x] = loss;
    partial[3 * blockIdx.x + 1] = vs;
    partial[3 * blockIdx.x + 2] = rs;
  }
}

// newton_finish_kernel for the job blockIdx.x: the mean is over the job's n_t rows
__global__ __launch_bounds__(kBlock) void newton_cv_finish_kernel(const CvCmd* __restrict__ cmd, const CvJob* __restrict__ jobs,
                                                                   const double* __restrict__ partial_all, double* __restrict__ sums_all,
                                                                   double* __restrict__ rec_all) {
  __shared__ double sh[kBlock];
  const int job = blockIdx.x;
  if (cmd[job].action == kCvIdle) return;
  const double* __restrict__ partial = partial_all + (size_t)job * 3 * kStateMaxBlocks;
  const int blocks = jobs[job].state_blocks;
  double s[3] = {0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < blocks; b += kBlock)
    for (int c = 0; c < 3; ++c) s[c] += partial[3 * b + c];
  for (int c = 0; c < 3; ++c) s[c] = block_sum(s[c], sh);
  if (threadIdx.x == 0) {
    rec_all[(size_t)job * kRecLen + kRecLoss] = s[0] / (double)jobs[job].n_t;
    sums_all[2 * job] = s[1];
    sums_all[2 * job + 1] = s[2];
  }
}

// newton_dense_tile_kernel for the job blockIdx.z: blockIdx.y is a chunk of the JOB's rows.  part[job][chunk][pair][tid].
__global__ __launch_bounds__(kBlock) void newton_cv_dense_tile_kernel(const CvCmd* __restrict__ cmd, const CvJob* __restrict__ jobs,
                                                                       const double* __restrict__ x, const double* __restrict__ v_all,
                                                                       const double* __restrict__ r_all, const double* __restrict__ mu_all,
                                                                       int64_t n, int p, int max_chunks, double* __restrict__ part) {
  __shared__ double A[kTileCols][kTileRows + 1], B[kTileCols][kTileRows + 1];
  const int job = blockIdx.z;
  if (cmd[job].action != kCvStep) return;
  const CvJob J = jobs[job];
  if ((int)blockIdx.y >= J.chunks) return;
  const double* __restrict__ mu = mu_all + (size_t)J.set * (size_t)p;
  const double* __restrict__ v = v_all + (size_t)job * (size_t)n;
  const double* __restrict__ r = r_all + (size_t)job * (size_t)n;
  const int tid = threadIdx.x, ncols = p + 2;
  const int T = (ncols + kTileCols - 1) / kTileCols;
  int pair = blockIdx.x, tj = 0;
  while (pair >= T - tj) {
    pair -= T - tj;
    ++tj;
  }
  const int tk = tj + pair;
  const int ta = tid & (kTileCols - 1), tb = tid / kTileCols;
  const int64_t r0 = (int64_t)blockIdx.y * J.rows_per_chunk;
  const int64_t r1 = r0 + J.rows_per_chunk < J.n_t ? r0 + J.rows_per_chunk : J.n_t;
  double acc = 0.0;
  for (int64_t base = r0; base < r1; base += kTileRows) {
    for (int e = tid; e < kTileCols * kTileRows; e += kBlock) {
      const int row = e & (kTileRows - 1), col = e / kTileRows;
      const int64_t li = base + row;
      const int ca = tj * kTileCols + col, cb = tk * kTileCols + col;
      double da = 0.0, db = 0.0;
      if (li < r1) {
        const int64_t i = cv_row(J, li);
        if (ca <= p) da = ca < p ? x[i + (int64_t)ca * n] - mu[ca] : 1.0;
        if (cb == p + 1) db = r[i];
        else if (cb <= p) db = v[i] * (cb < p ? x[i + (int64_t)cb * n] - mu[cb] : 1.0);
      }
      A[col][row] = da;
      B[col][row] = db;
    }
    __syncthreads();
    for (int i = 0; i < kTileRows; ++i) acc += A[ta][i] * B[tb][i];
    __syncthreads();
  }
  part[(((size_t)job * (size_t)max_chunks + blockIdx.y) * gridDim.x + blockIdx.x) * kBlock + tid] = acc;
}

// cov_reduce_kernel for the job blockIdx.y: its chunks added in chunk order into M[job]
__global__ __launch_bounds__(kBlock) void newton_cv_reduce_kernel(const CvCmd* __restrict__ cmd, const CvJob* __restrict__ jobs,
                                                                   const double* __restrict__ part, int max_chunks, int ncols,
                                                                   double* __restrict__ M_all) {
  const int job = blockIdx.y;
  if (cmd[job].action != kCvStep) return;
  const int tid = threadIdx.x;
  const int T = (ncols + kTileCols - 1) / kTileCols;
  int pair = blockIdx.x, tj = 0;
  while (pair >= T - tj) {
    pair -= T - tj;
    ++tj;
  }
  const int tk = tj + pair;
  const int a = tj * kTileCols + (tid & (kTileCols - 1)), b = tk * kTileCols + tid / kTileCols;
  if (a >= ncols || b >= ncols) return;
  const int chunks = jobs[job].chunks;
  double* __restrict__ M = M_all + (size_t)job * (size_t)ncols * (size_t)ncols;
  double s = 0.0;
  for (int c = 0; c < chunks; ++c) s += part[(((size_t)job * (size_t)max_chunks + c) * gridDim.x + blockIdx.x) * kBlock + tid];
  M[(size_t)a * ncols + b] = s;
  if (tj != tk) M[(size_t)b * ncols + a] = s;
}

// The entries of a column in the rows of a training set: two ranges of positions (cut: NewtonCvProblem), entry e of the
// set at position at(e).  find(row): the position of the entry in that row, or -1.
struct CvColumn {
  int a0, a1, b0, b1;
  __device__ CvColumn(const int32_t* __restrict__ cut, int n_sets, int j, int group, bool rest) {
    const int32_t* c = cut + (size_t)j * (size_t)(n_sets + 1);
    if (rest) {
      a0 = c[0];
      a1 = c[group];
      b0 = c[group + 1];
      b1 = c[n_sets];
    } else {
      a0 = c[group];
      a1 = c[group + 1];
      b0 = b1 = a1;
    }
  }
  __device__ int count() const { return (a1 - a0) + (b1 - b0); }
  __device__ int at(int e) const { return e < a1 - a0 ? a0 + e : b0 + (e - (a1 - a0)); }
  // split: the first row of the second range of rows (rows below it can only sit in the first range of positions)
  __device__ int find(const int32_t* __restrict__ rowidx, int32_t row, int64_t split) const {
    const bool first = (int64_t)row < split;
    const int lo = first ? a0 : b0, hi = first ? a1 : b1;
    const int pos = lower_bound_row(rowidx, lo, hi, row);
    return pos < hi && rowidx[pos] == row ? pos : -1;
  }
};

// newton_sparse_pair_kernel for the job blockIdx.z over the entries in the rows of its training set
__global__ __launch_bounds__(kBlock) void newton_cv_sparse_pair_kernel(const CvCmd* __restrict__ cmd, const CvJob* __restrict__ jobs,
                                                                        const int32_t* __restrict__ cut, int n_sets, int rest,
                                                                        const int32_t* __restrict__ rowidx, const double* __restrict__ val,
                                                                        const double* __restrict__ v_all, const double* __restrict__ r_all,
                                                                        const double* __restrict__ mu_all, const double* __restrict__ sums_all,
                                                                        int64_t n, int p, double* __restrict__ M_all) {
  __shared__ double sh[kBlock];
  const int job = blockIdx.z;
  if (cmd[job].action != kCvStep) return;
  const int j = blockIdx.x, k = blockIdx.y, nc = p + 2, tid = threadIdx.x;
  if (k < j) return;
  const CvJob J = jobs[job];
  const double* __restrict__ mu = mu_all + (size_t)J.set * (size_t)p;
  const double* __restrict__ v = v_all + (size_t)job * (size_t)n;
  const double* __restrict__ r = r_all + (size_t)job * (size_t)n;
  const double* __restrict__ sums = sums_all + 2 * (size_t)job;
  double* __restrict__ M = M_all + (size_t)job * (size_t)nc * (size_t)nc;
  const int64_t split = J.b0;           // (training on the own group: b0 = a1, past every row of the set)
  const CvColumn cj(cut, n_sets, j, J.set, rest != 0);
  const int nj = cj.count();
  const double mj = mu[j];
  const bool j_full = (int64_t)nj == J.n_t;
  if (k >= p) {                                  // against the ones (weights v) or q (weights r)
    const double* wt = k == p ? v : r;
    double a = 0.0, ws = 0.0;
    for (int e = tid; e < nj; e += kBlock) {
      const int q = cj.at(e);
      const double wi = wt[rowidx[q]];
      a += wi * (val[q] - mj);
      ws += wi;
    }
    a = block_sum(a, sh);
    ws = block_sum(ws, sh);
    if (tid == 0) {
      const double total = sums[k - p];
      M[(size_t)j * nc + k] = a - mj * (j_full ? 0.0 : total - ws);
      if (j == 0) M[(size_t)p * nc + k] = total;
    }
    return;
  }
  const CvColumn ck(cut, n_sets, k, J.set, rest != 0);
  const int nk = ck.count();
  const double mk = mu[k];
  double both = 0.0, only_j = 0.0, only_k = 0.0, v_union = 0.0;
  for (int e = tid; e < nj; e += kBlock) {
    const int q = cj.at(e);
    const int32_t row = rowidx[q];
    const double vi = v[row], d = val[q] - mj;
    v_union += vi;
    const int pos = j == k ? q : ck.find(rowidx, row, split);
    if (pos >= 0) both += vi * d * (val[pos] - mk);
    else only_j += vi * d;
  }
  if (j != k)
    for (int e = tid; e < nk; e += kBlock) {
      const int s = ck.at(e);
      const int32_t row = rowidx[s];
      if (cj.find(rowidx, row, split) < 0) {
        const double vi = v[row];
        only_k += vi * (val[s] - mk);
        v_union += vi;
      }
    }
  both = block_sum(both, sh);
  only_j = block_sum(only_j, sh);
  only_k = block_sum(only_k, sh);
  v_union = block_sum(v_union, sh);
  if (tid == 0) {
    const bool full = j_full || (int64_t)nk == J.n_t;
    const double in_neither = full ? 0.0 : sums[0] - v_union;
    M[(size_t)j * nc + k] = both - mk * only_j - mj * only_k + in_neither * mj * mk;
  }
}

// newton_blend_kernel for the job blockIdx.x: a halving (t = 1/2), or the path's start published as it is (t = 1)
__global__ __launch_bounds__(64) void newton_cv_blend_kernel(const CvCmd* __restrict__ cmd, const CvJob* __restrict__ jobs,
                                                              const double* __restrict__ scale_all, int p, double* __restrict__ u_all,
                                                              double* __restrict__ a_all, double* __restrict__ rec_all) {
  __shared__ double un[kNewtonMaxFeatures + 1];
  const int job = blockIdx.x, P = p + 1;
  const CvCmd c = cmd[job];
  if (c.action != kCvHalve && c.action != kCvStart) return;
  const double* __restrict__ u_cur = u_all + ((size_t)job * 2 + (size_t)c.cur) * (size_t)P;
  double* __restrict__ u_cand = u_all + ((size_t)job * 2 + (size_t)(1 - c.cur)) * (size_t)P;
  const double t = c.action == kCvStart ? 1.0 : 0.5;
  for (int k = threadIdx.x; k <= p; k += 64) un[k] = t == 1.0 ? u_cand[k] : u_cur[k] + t * (u_cand[k] - u_cur[k]);
  __syncthreads();
  publish_candidate(un, u_cur, scale_all + (size_t)jobs[job].set * (size_t)p, p, u_cand, a_all + (size_t)job * (size_t)P,
                    rec_all + (size_t)job * kRecLen);
}

// newton_cd_kernel for the job blockIdx.x: one wavefront per job, each declaring the whole LDS, so the jobs spread one
// per CU.  Before anything else it stores the current iterate into U[slot] where the host says it answers a lambda.
__global__ __launch_bounds__(64) void newton_cv_cd_kernel(const CvCmd* __restrict__ cmd, const CvJob* __restrict__ jobs,
                                                           const double* __restrict__ M_all, const double* __restrict__ scale_all, int p,
                                                           int n_lambda, int fit_intercept, unsigned max_sweeps, double tol,
                                                           double* __restrict__ u_all, double* __restrict__ a_all,
                                                           double* __restrict__ rec_all, double* __restrict__ U_all) {
  __shared__ double lds[newton_state_doubles(kNewtonMaxFeatures)];
  const int job = blockIdx.x, P = p + 1, nc = p + 2;
  const CvCmd c = cmd[job];
  const double* __restrict__ u_cur = u_all + ((size_t)job * 2 + (size_t)c.cur) * (size_t)P;
  if (c.slot >= 0) {
    double* __restrict__ U = U_all + ((size_t)job * (size_t)n_lambda + (size_t)c.slot) * (size_t)P;
    for (int k = threadIdx.x; k < P; k += 64) U[k] = u_cur[k];
  }
  if (c.action != kCvStep) return;
  newton_cd_solve(lds, M_all + (size_t)job * (size_t)nc * (size_t)nc, scale_all + (size_t)jobs[job].set * (size_t)p, p,
                  (double)jobs[job].n_t, u_cur, c.l2, c.l1, c.ridge, fit_intercept, max_sweeps, tol,
                  u_all + ((size_t)job * 2 + (size_t)(1 - c.cur)) * (size_t)P, a_all + (size_t)job * (size_t)P,
                  rec_all + (size_t)job * kRecLen);
}

// ---- wide cross-validation (wnewton_cv_run): the wide kernels with a job dimension ----
// The state, finish, dense tile and reduce kernels are the ones above, on the row chunks wnewton_run would choose for n_t
// rows (CvGeometry).  Every job has its own H (leading dimension ld = wide_leading_dim(P)), diag H and q.

// wide_scale_kernel on a grid of (column, job): the job's M into its H, diag H and q, with its training set's scales and n_t
__global__ __launch_bounds__(kBlock) void newton_cv_wide_scale_kernel(const CvCmd* __restrict__ cmd, const CvJob* __restrict__ jobs,
                                                                       const double* __restrict__ M_all, const double* __restrict__ scale_all,
                                                                       int p, int ld, double* __restrict__ H_all, double* __restrict__ Hd_all,
                                                                       double* __restrict__ q_all) {
  const int job = blockIdx.y;
  if (cmd[job].action != kCvStep) return;
  const int j = blockIdx.x, P = p + 1, ncols = p + 2;
  const double* __restrict__ M = M_all + (size_t)job * (size_t)ncols * (size_t)ncols;
  const double* __restrict__ scale = scale_all + (size_t)jobs[job].set * (size_t)p;
  double* __restrict__ A = H_all + (size_t)job * (size_t)ld * (size_t)P;
  const double dn = (double)jobs[job].n_t;
  const double sj = j < p ? scale[j] : 1.0;
  for (int k = threadIdx.x; k < ld; k += kBlock) {
    double v = 0.0;
    if (k < P) {
      const double sk = k < p ? scale[k] : 1.0;
      v = k >= j ? M[(size_t)j * ncols + k] / dn / (sj * sk) : M[(size_t)k * ncols + j] / dn / (sk * sj);
    }
    A[(size_t)j * ld + k] = v;
    if (k == j) Hd_all[(size_t)job * (size_t)P + j] = v;
  }
  if (threadIdx.x == 0) q_all[(size_t)job * (size_t)P + j] = M[(size_t)j * ncols + P] / dn / sj;
}

// newton_wide_blend_kernel for the job blockIdx.x: a halving (t = 1/2), or the path's start published as it is (t = 1)
__global__ __launch_bounds__(64) void newton_cv_wide_blend_kernel(const CvCmd* __restrict__ cmd, const CvJob* __restrict__ jobs,
                                                                   const double* __restrict__ scale_all, int p, double* u_all,
                                                                   double* __restrict__ a_all, double* __restrict__ rec_all) {
  const int job = blockIdx.x, P = p + 1;
  const CvCmd c = cmd[job];
  if (c.action != kCvHalve && c.action != kCvStart) return;
  const double* u_cur = u_all + ((size_t)job * 2 + (size_t)c.cur) * (size_t)P;
  double* u_cand = u_all + ((size_t)job * 2 + (size_t)(1 - c.cur)) * (size_t)P;
  publish_candidate(BlendedCandidate{u_cur, u_cand, c.action == kCvStart ? 1.0 : 0.5}, u_cur,
                    scale_all + (size_t)jobs[job].set * (size_t)p, p, u_cand, a_all + (size_t)job * (size_t)P,
                    rec_all + (size_t)job * kRecLen);
}

// newton_wide_cd_kernel for the job blockIdx.x: one workgroup per job, each declaring the whole LDS, so the jobs spread one
// per CU (more jobs than CUs queue: no workgroup waits for another).  Before anything else it stores the current iterate
// into U[slot] where the host says it answers a lambda.
template <int kWidth>
__global__ __launch_bounds__(kWidth) void newton_cv_wide_cd_kernel(const CvCmd* __restrict__ cmd, const CvJob* __restrict__ jobs,
                                                                    const double* __restrict__ H_all, const double* __restrict__ Hd_all,
                                                                    const double* __restrict__ q_all, const double* __restrict__ scale_all,
                                                                    int p, int ld, int n_lambda, int fit_intercept, unsigned max_sweeps,
                                                                    double tol, double* __restrict__ u_all, double* __restrict__ a_all,
                                                                    double* __restrict__ rec_all, double* __restrict__ U_all) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[kWnewtonLdsBytes];
  const int job = blockIdx.x, P = p + 1;
  const CvCmd c = cmd[job];
  const double* __restrict__ u_cur = u_all + ((size_t)job * 2 + (size_t)c.cur) * (size_t)P;
  if (c.slot >= 0) {
    double* __restrict__ U = U_all + ((size_t)job * (size_t)n_lambda + (size_t)c.slot) * (size_t)P;
    for (int k = threadIdx.x; k < P; k += kWidth) U[k] = u_cur[k];
  }
  if (c.action != kCvStep) return;
  newton_wide_cd_solve<kWidth>(lds, H_all + (size_t)job * (size_t)ld * (size_t)P, Hd_all + (size_t)job * (size_t)P,
                               q_all + (size_t)job * (size_t)P, scale_all + (size_t)jobs[job].set * (size_t)p, p, ld, u_cur, c.l2, c.l1,
                               c.ridge, fit_intercept, max_sweeps, tol, u_all + ((size_t)job * 2 + (size_t)(1 - c.cur)) * (size_t)P,
                               a_all + (size_t)job * (size_t)P, rec_all + (size_t)job * kRecLen);
}

struct Stream {
  hipStream_t st = nullptr;
  hipEvent_t e[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // (e[4]: the wide mode's scale kernel)
  double* rec_host = nullptr;          // pinned: the record of a state pass
  DeviceSetup S;                       // sparse x: the sample-major copy (the feature-major one lives in the arena)
  ~Stream() {
    S.release();
    for (hipEvent_t v : e)
      if (v) (void)hipEventDestroy(v);
    if (rec_host) (void)hipHostFree(rec_host);
    if (st) (void)hipStreamDestroy(st);
  }
};

// What one problem keeps on the device and the launches of an outer step as named host steps.  newton_run (a fit) and
// newton_probe (diagnostics) both go through these: the same kernels on the same grids in the same order.
struct NewtonDevice {
  int64_t n = 0, nnz = 0;
  int p = 0, P = 0, nc = 0;
  bool sparse = false, centre = true, timed = false;
  // the wide mode (wnewton_run; set before setup): H, diag H and q in global memory, the inner solve on `width` lanes,
  // the row chunks of wide_layout.hpp's wide_row_chunks
  bool wide = false;
  int width = 0, ld = 0;
  double *d_H = nullptr, *d_Hd = nullptr, *d_q = nullptr;
  // dense x: the tile pairs and the row chunks (a function of n and p alone)
  int pairs = 0;
  int64_t rows_per_chunk = 0, chunks = 0;
  int state_blocks = 0;
  Arena A;
  Stream sx;
  hipStream_t st = nullptr;
  double *d_x = nullptr, *d_y = nullptr, *d_v = nullptr, *d_r = nullptr, *d_mu = nullptr, *d_scale = nullptr, *d_part = nullptr,
         *d_M = nullptr, *d_partial = nullptr, *d_sums = nullptr, *d_rec = nullptr, *d_a = nullptr, *d_cur = nullptr, *d_cand = nullptr,
         *d_U = nullptr;
  int32_t *d_colptr = nullptr, *d_rowidx = nullptr;
  const double* rec = nullptr;         // the pinned copy of the record, as of the last state pass
  double passes = 0.0;
  float state_ms = 0.f;

  // setup and upload: x (cols: its columns with ascending rows), y and scale; the iterate and the candidate start as
  // u_cur0 and u_cand0 (p + 1 values each, host memory that outlives the call); the column means
  int setup(const NewtonProblem& pb, const AscendingColumns& cols, const double* u_cur0, const double* u_cand0, bool timed_) {
    n = pb.n;
    p = (int)pb.p;
    P = p + 1;
    nc = p + 2;
    sparse = pb.x_dense == nullptr;
    centre = pb.centre;
    timed = timed_;
    const int L = pb.n_lambda;
    SGD_HIP_TRY(hipSetDevice(pb.device));
    nnz = sparse ? pb.colptr[p] : 0;
    const int T = (nc + kTileCols - 1) / kTileCols;
    pairs = T * (T + 1) / 2;
    rows_per_chunk = wide ? wide_rows_per_chunk(n, nc, kTileRows)
                          : dense_rows_per_chunk(n, pairs);
    chunks = (n + rows_per_chunk - 1) / rows_per_chunk;
    state_blocks = (int)std::min<int64_t>(kStateMaxBlocks, (n + kBlock - 1) / kBlock);
    ld = (int)wide_leading_dim(P);

    const size_t o_x = A.reserve(sizeof(double) * (size_t)(sparse ? nnz : n * (int64_t)p));
    const size_t o_colptr = A.reserve(sparse ? sizeof(int32_t) * (size_t)P : 0);
    const size_t o_rowidx = A.reserve(sparse ? sizeof(int32_t) * (size_t)nnz : 0);
    const size_t o_y = A.reserve(sizeof(double) * (size_t)n);
    const size_t o_v = A.reserve(sizeof(double) * (size_t)n);
    const size_t o_r = A.reserve(sizeof(double) * (size_t)n);
    const size_t o_mu = A.reserve(sizeof(double) * (size_t)nc);          // cov_sum_kernel: the means, then the sum and the mean of y
    const size_t o_scale = A.reserve(sizeof(double) * (size_t)p);
    const size_t o_part = A.reserve(sparse ? 0 : sizeof(double) * (size_t)(chunks * pairs * kBlock));
    const size_t o_M = A.reserve(sizeof(double) * (size_t)nc * (size_t)nc);
    const size_t o_partial = A.reserve(sizeof(double) * 3 * (size_t)state_blocks);
    const size_t o_sums = A.reserve(sizeof(double) * 2);
    const size_t o_rec = A.reserve(sizeof(double) * kRecLen);
    const size_t o_u0 = A.reserve(sizeof(double) * (size_t)P);
    const size_t o_u1 = A.reserve(sizeof(double) * (size_t)P);
    const size_t o_a = A.reserve(sizeof(double) * (size_t)P);
    const size_t o_U = A.reserve(sizeof(double) * (size_t)L * (size_t)P);
    const size_t o_H = A.reserve(wide ? sizeof(double) * (size_t)ld * (size_t)P : 0);
    const size_t o_Hd = A.reserve(wide ? sizeof(double) * (size_t)P : 0);
    const size_t o_q = A.reserve(wide ? sizeof(double) * (size_t)P : 0);
    SGD_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&A.base), A.used));

    SGD_HIP_TRY(hipStreamCreateWithFlags(&sx.st, hipStreamNonBlocking));
    SGD_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&sx.rec_host), sizeof(double) * kRecLen, hipHostMallocDefault));
    if (timed)
      for (hipEvent_t& e : sx.e) SGD_HIP_TRY(hipEventCreate(&e));
    st = sx.st;
    rec = sx.rec_host;
    d_x = A.at<double>(o_x);
    d_colptr = A.at<int32_t>(o_colptr);
    d_rowidx = A.at<int32_t>(o_rowidx);
    d_y = A.at<double>(o_y);
    d_v = A.at<double>(o_v);
    d_r = A.at<double>(o_r);
    d_mu = A.at<double>(o_mu);
    d_scale = A.at<double>(o_scale);
    d_part = A.at<double>(o_part);
    d_M = A.at<double>(o_M);
    d_partial = A.at<double>(o_partial);
    d_sums = A.at<double>(o_sums);
    d_rec = A.at<double>(o_rec);
    d_a = A.at<double>(o_a);
    d_cur = A.at<double>(o_u0);
    d_cand = A.at<double>(o_u1);
    d_U = A.at<double>(o_U);
    d_H = A.at<double>(o_H);
    d_Hd = A.at<double>(o_Hd);
    d_q = A.at<double>(o_q);
    if (sparse) {
      if (nnz > 0) {
        SGD_HIP_TRY(hipMemcpyAsync(d_x, cols.values, sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice, st));
        SGD_HIP_TRY(hipMemcpyAsync(d_rowidx, cols.rowidx, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice, st));
      }
      SGD_HIP_TRY(hipMemcpyAsync(d_colptr, pb.colptr, sizeof(int32_t) * (size_t)P, hipMemcpyHostToDevice, st));
      DeviceSetup& S = sx.S;
      S.n = n;
      S.p = p;
      S.nnz = nnz;
      if (nnz > 0) {
        S.colptr = d_colptr;
        S.rowidx = d_rowidx;
        S.val = d_x;
        const int rc = device_transpose(S, st);
        S.colptr = S.rowidx = nullptr;               // the arena owns the feature-major copy; S the sample-major one
        S.val = nullptr;
        if (rc) return rc;
      } else {                                       // nothing stored: every row is empty
        SGD_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&S.sptr), sizeof(int64_t) * ((size_t)n + 1)));
        SGD_HIP_TRY(hipMemsetAsync(S.sptr, 0, sizeof(int64_t) * ((size_t)n + 1), st));
      }
    } else {
      SGD_HIP_TRY(hipMemcpyAsync(d_x, pb.x_dense, sizeof(double) * (size_t)(n * (int64_t)p), hipMemcpyHostToDevice, st));
    }
    SGD_HIP_TRY(hipMemcpyAsync(d_y, pb.y, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
    SGD_HIP_TRY(hipMemcpyAsync(d_scale, pb.scale, sizeof(double) * (size_t)p, hipMemcpyHostToDevice, st));
    SGD_HIP_TRY(hipMemcpyAsync(d_cur, u_cur0, sizeof(double) * (size_t)P, hipMemcpyHostToDevice, st));
    SGD_HIP_TRY(hipMemcpyAsync(d_cand, u_cand0, sizeof(double) * (size_t)P, hipMemcpyHostToDevice, st));
    SGD_HIP_TRY(hipMemsetAsync(d_rec, 0, sizeof(double) * kRecLen, st));
    if (sparse)
      hipLaunchKernelGGL(cov_sum_kernel<true>, dim3((unsigned)P), dim3(kBlock), 0, st, d_x, d_colptr, d_y, n, p, 1, centre ? 1 : 0, d_mu);
    else
      hipLaunchKernelGGL(cov_sum_kernel<false>, dim3((unsigned)P), dim3(kBlock), 0, st, d_x, (const int32_t*)nullptr, d_y, n, p,
                         1, centre ? 1 : 0, d_mu);
    SGD_HIP_TRY(hipGetLastError());
    return SGDNET_OK;
  }

  // publish / blend: d_cand <- d_cur + t (d_cand - d_cur), its state-pass form d_a and its record
  int publish(double t) {
    if (wide) hipLaunchKernelGGL(newton_wide_blend_kernel, dim3(1), dim3(64), 0, st, d_cur, d_scale, p, t, d_cand, d_a, d_rec);
    else hipLaunchKernelGGL(newton_blend_kernel, dim3(1), dim3(64), 0, st, d_cur, d_scale, p, t, d_cand, d_a, d_rec);
    SGD_HIP_TRY(hipGetLastError());
    return SGDNET_OK;
  }

  // the state pass at the candidate (d_a) and its record, read back into rec
  int state_pass() {
    if (timed) SGD_HIP_TRY(hipEventRecord(sx.e[2], st));
    if (sparse)
      hipLaunchKernelGGL(newton_state_kernel<true>, dim3((unsigned)state_blocks), dim3(kBlock), 0, st, sx.S.sval, sx.S.sptr, sx.S.sidx, d_y,
                         d_mu, d_a, n, p, centre ? 1 : 0, d_v, d_r, d_partial);
    else
      hipLaunchKernelGGL(newton_state_kernel<false>, dim3((unsigned)state_blocks), dim3(kBlock), 0, st, d_x, (const int64_t*)nullptr,
                         (const int32_t*)nullptr, d_y, d_mu, d_a, n, p, 1, d_v, d_r, d_partial);
    hipLaunchKernelGGL(newton_finish_kernel, dim3(1), dim3(kBlock), 0, st, d_partial, state_blocks, n, d_sums, d_rec);
    SGD_HIP_TRY(hipGetLastError());
    if (timed) SGD_HIP_TRY(hipEventRecord(sx.e[3], st));
    SGD_HIP_TRY(hipMemcpyAsync(sx.rec_host, d_rec, sizeof(double) * kRecLen, hipMemcpyDeviceToHost, st));
    SGD_HIP_TRY(hipStreamSynchronize(st));
    passes += 1.0;
    if (timed) {
      float ms = 0.f;
      SGD_HIP_TRY(hipEventElapsedTime(&ms, sx.e[2], sx.e[3]));
      state_ms += ms;
    }
    return SGDNET_OK;
  }

  // the moments pass: d_M from d_v, d_r and the sums of the last state pass (timed: between the events 0 and 1)
  int moments() {
    if (timed) SGD_HIP_TRY(hipEventRecord(sx.e[0], st));
    if (sparse) {
      hipLaunchKernelGGL(newton_sparse_pair_kernel, dim3((unsigned)p, (unsigned)nc), dim3(kBlock), 0, st, d_colptr, d_rowidx, d_x, d_v,
                         d_r, d_mu, d_sums, n, p, d_M);
    } else {
      hipLaunchKernelGGL(newton_dense_tile_kernel, dim3((unsigned)pairs, (unsigned)chunks), dim3(kBlock), 0, st, d_x, d_v, d_r, d_mu, n,
                         p, rows_per_chunk, d_part);
      hipLaunchKernelGGL(cov_reduce_kernel, dim3((unsigned)pairs), dim3(kBlock), 0, st, d_part, (int)chunks, (const int32_t*)nullptr, nc,
                         d_M);
    }
    SGD_HIP_TRY(hipGetLastError());
    if (timed) SGD_HIP_TRY(hipEventRecord(sx.e[1], st));
    return SGDNET_OK;
  }

  // wide: H, diag H and q from d_M (timed: up to the event 4)
  int wide_scale() {
    hipLaunchKernelGGL(wide_scale_kernel, dim3((unsigned)P), dim3(kBlock), 0, st, d_M, d_scale, p, p + 2, ld, (double)n, d_H, d_Hd, d_q);
    SGD_HIP_TRY(hipGetLastError());
    if (timed) SGD_HIP_TRY(hipEventRecord(sx.e[4], st));
    return SGDNET_OK;
  }

  // wide: the list solve on d_H, d_Hd and d_q about d_cur
  int wide_solve(double al, double be, bool ridge, bool fit_intercept, unsigned max_sweeps, double tol) {
    const auto kernel = width == kWideNarrow ? newton_wide_cd_kernel<kWideNarrow> : newton_wide_cd_kernel<kWideFull>;
    hipLaunchKernelGGL(kernel, dim3(1), dim3((unsigned)width), 0, st, d_H, d_Hd, d_q, d_scale, p, ld, d_cur, al, be, ridge ? 1 : 0,
                       fit_intercept ? 1 : 0, max_sweeps, tol, d_cand, d_a, d_rec);
    SGD_HIP_TRY(hipGetLastError());
    return SGDNET_OK;
  }

  // the inner solve on d_M about d_cur: the candidate into d_cand and d_a, its record into d_rec
  int inner_solve(double al, double be, bool ridge, bool fit_intercept, unsigned max_sweeps, double tol) {
    if (wide) {                          // scale, then the solve on H about d_cur
      const int rc = wide_scale();
      return rc ? rc : wide_solve(al, be, ridge, fit_intercept, max_sweeps, tol);
    }
    hipLaunchKernelGGL(newton_cd_kernel, dim3(1), dim3(64), 0, st, d_M, d_scale, p, (double)n, d_cur, al, be, ridge ? 1 : 0,
                       fit_intercept ? 1 : 0, max_sweeps, tol, d_cand, d_a, d_rec);
    SGD_HIP_TRY(hipGetLastError());
    return SGDNET_OK;
  }
};

}  // namespace

namespace {

// newton_run and wnewton_run: one outer loop, one state machine.  wide: NewtonDevice scales the moments into H in global
// memory and runs newton_wide_cd_kernel<width>; the dense row chunks follow wide_row_chunks; the blend has no array of
// kNewtonMaxFeatures + 1.  Not wide: exactly the launches Newton mode has always made.
int newton_loop(const NewtonProblem& pb, bool timed, NewtonResult* out, bool wide, int width) {
  const int p = (int)pb.p, P = p + 1, L = pb.n_lambda;
  const bool sparse = pb.x_dense == nullptr;
  if (pb.n <= 0 || pb.p <= 0 || pb.p > (wide ? kWnewtonMaxFeatures : kNewtonMaxFeatures) || L <= 0 ||
      (wide && (sparse || (width != kWideNarrow && width != kWideFull))) || !pb.y || !pb.scale || !pb.alpha || !pb.beta || pb.max_iter == 0 ||
      (!sparse && pb.colptr) || (sparse && (!pb.colptr || !pb.rowidx || !pb.values))) {
    set_error("%s: invalid problem", wide ? "wnewton_run" : "newton_run");
    return SGDNET_EINVAL;
  }
  const int32_t* no_rows = nullptr;
  const AscendingColumns cols(sparse ? pb.colptr : no_rows, pb.rowidx, pb.values, sparse ? p : 0);
  std::vector<double> start((size_t)P, 0.0);
  start[(size_t)p] = pb.b0;
  NewtonDevice D;
  D.wide = wide;
  D.width = width;
  int rc = D.setup(pb, cols, start.data(), start.data(), timed);
  if (rc) return rc;
  hipStream_t st = D.st;

  out->passes = out->sweeps = out->halvings = 0.0;
  out->state_ms = out->moments_ms = out->cd_ms = out->scale_ms = 0.f;
  const double* rec = D.rec;
  // the path's start: w = 0, b = b0
  rc = D.publish(1.0);
  if (!rc) rc = D.state_pass();
  if (rc) return rc;
  double loss = rec[kRecLoss], half_sq = rec[kRecHalfSq], abs1 = rec[kRecAbs];

  out->loss.assign((size_t)L, 0.0);
  out->steps.assign((size_t)L, 0);
  out->unconverged.assign((size_t)L, 0);
  for (int l = 0; l < L; ++l) {
    const double al = pb.alpha[l], be = pb.ridge ? 0.0 : pb.beta[l];
    double objective = loss + al * half_sq + be * abs1;
    unsigned steps = 0;
    bool converged = false;
    while (steps < pb.max_iter && !converged) {
      if ((rc = D.moments()) || (rc = D.inner_solve(al, be, pb.ridge, pb.fit_intercept, kNewtonMaxSweeps, pb.tol)) || (rc = D.state_pass()))
        return rc;
      if (timed) {
        float ms = 0.f;
        SGD_HIP_TRY(hipEventElapsedTime(&ms, D.sx.e[0], D.sx.e[1]));
        out->moments_ms += ms;
        if (wide) {
          SGD_HIP_TRY(hipEventElapsedTime(&ms, D.sx.e[1], D.sx.e[4]));
          out->scale_ms += ms;
        }
        SGD_HIP_TRY(hipEventElapsedTime(&ms, D.sx.e[wide ? 4 : 1], D.sx.e[2]));
        out->cd_ms += ms;
      }
      out->sweeps += rec[kRecSweeps];
      bool negligible = rec[kRecNegligible] != 0.0;
      double candidate = rec[kRecLoss] + al * rec[kRecHalfSq] + be * rec[kRecAbs];
      // (a candidate whose objective is not a number counts as one that rose)
      for (int h = 0; h < kNewtonMaxHalvings && rec[kRecChange] > 0.0 && !(candidate <= objective + kNewtonObjectiveSlack * fabs(objective)); ++h) {
        if ((rc = D.publish(0.5)) || (rc = D.state_pass())) return rc;
        candidate = rec[kRecLoss] + al * rec[kRecHalfSq] + be * rec[kRecAbs];
        out->halvings += 1.0;
        negligible = false;              // (the inner solve said so of the whole step, not of a part of it)
      }
      std::swap(D.d_cur, D.d_cand);
      objective = candidate;
      loss = rec[kRecLoss];
      half_sq = rec[kRecHalfSq];
      abs1 = rec[kRecAbs];
      ++steps;
      const double change = rec[kRecChange], size = rec[kRecSize];
      const bool all_zero = size == 0.0 && change == 0.0;
      const bool no_change = size != 0.0 && change / size <= pb.tol;
      converged = rec[kRecInnerConverged] != 0.0 && (all_zero || no_change || negligible);
    }
    SGD_HIP_TRY(hipMemcpyAsync(D.d_U + (size_t)l * (size_t)P, D.d_cur, sizeof(double) * (size_t)P, hipMemcpyDeviceToDevice, st));
    out->loss[(size_t)l] = loss;
    out->steps[(size_t)l] = (int32_t)steps;
    out->unconverged[(size_t)l] = converged ? 0 : 1;
  }
  out->passes = D.passes;
  out->state_ms = D.state_ms;

  out->mean.resize((size_t)p);
  out->u.resize((size_t)L * (size_t)P);
  SGD_HIP_TRY(hipMemcpyAsync(out->mean.data(), D.d_mu, sizeof(double) * (size_t)p, hipMemcpyDeviceToHost, st));
  SGD_HIP_TRY(hipMemcpyAsync(out->u.data(), D.d_U, sizeof(double) * (size_t)L * (size_t)P, hipMemcpyDeviceToHost, st));
  SGD_HIP_TRY(hipStreamSynchronize(st));
  return SGDNET_OK;
}

}  // namespace

int newton_run(const NewtonProblem& pb, bool timed, NewtonResult* out) { return newton_loop(pb, timed, out, false, 0); }

int wnewton_run(const NewtonProblem& pb, bool timed, NewtonResult* out, int width) {
  return newton_loop(pb, timed, out, true, width != 0 ? width : wide_cd_width((int)std::min<int64_t>(pb.p, kWnewtonMaxFeatures)));
}

// Diagnostics (include/sgdnet_hip.h): one outer step through the steps above, every output copied back.  The state is
// taken at the candidate io->u; the moments are those of that state; the inner solve runs on them about io->u_cur.
// wide (sgdnet_wnewton_probe): the steps of a wide fit, and what the scale kernel wrote is copied between it and the solve.
namespace {

template <class IO>
int newton_probe_steps(const NewtonProblem& pb, IO* io, bool wide, int width, double* H_out, double* Hd_out, double* q_out) {
  const int p = (int)pb.p, P = p + 1, nc = p + 2;
  const int64_t n = pb.n;
  const bool sparse = pb.x_dense == nullptr;
  const int32_t* no_rows = nullptr;
  const AscendingColumns cols(sparse ? pb.colptr : no_rows, pb.rowidx, pb.values, sparse ? p : 0);
  NewtonDevice D;
  D.wide = wide;
  D.width = width;
  int rc = D.setup(pb, cols, io->u_cur, io->u, false);
  if (rc) return rc;
  hipStream_t st = D.st;
  double rec[kRecLen];
  // a candidate as it was published: itself, its state-pass form and fields of the record
  auto fetch = [&](double* u_out, double* a_out, double* rec_out, int rec_from, int rec_len) -> int {
    if (u_out) SGD_HIP_TRY(hipMemcpyAsync(u_out, D.d_cand, sizeof(double) * (size_t)P, hipMemcpyDeviceToHost, st));
    if (a_out) SGD_HIP_TRY(hipMemcpyAsync(a_out, D.d_a, sizeof(double) * (size_t)P, hipMemcpyDeviceToHost, st));
    SGD_HIP_TRY(hipMemcpyAsync(rec, D.d_rec, sizeof(double) * kRecLen, hipMemcpyDeviceToHost, st));
    SGD_HIP_TRY(hipStreamSynchronize(st));
    std::copy(rec + rec_from, rec + rec_from + rec_len, rec_out);
    return SGDNET_OK;
  };
  if ((rc = D.publish(1.0)) || (rc = fetch(io->pub_u, io->pub_a, io->pub_rec, kRecHalfSq, 4))) return rc;
  if (io->mean) SGD_HIP_TRY(hipMemcpyAsync(io->mean, D.d_mu, sizeof(double) * (size_t)p, hipMemcpyDeviceToHost, st));
  if ((rc = D.state_pass())) return rc;
  io->loss = D.rec[kRecLoss];
  double sums[2];
  SGD_HIP_TRY(hipMemcpyAsync(sums, D.d_sums, sizeof(sums), hipMemcpyDeviceToHost, st));
  if (io->v) SGD_HIP_TRY(hipMemcpyAsync(io->v, D.d_v, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
  if (io->r) SGD_HIP_TRY(hipMemcpyAsync(io->r, D.d_r, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
  if ((rc = D.moments())) return rc;
  if (io->M) SGD_HIP_TRY(hipMemcpyAsync(io->M, D.d_M, sizeof(double) * (size_t)nc * (size_t)nc, hipMemcpyDeviceToHost, st));
  const double be = io->ridge ? 0.0 : io->l1;
  if (wide) {
    if ((rc = D.wide_scale())) return rc;
    if (H_out) SGD_HIP_TRY(hipMemcpyAsync(H_out, D.d_H, sizeof(double) * (size_t)D.ld * (size_t)P, hipMemcpyDeviceToHost, st));
    if (Hd_out) SGD_HIP_TRY(hipMemcpyAsync(Hd_out, D.d_Hd, sizeof(double) * (size_t)P, hipMemcpyDeviceToHost, st));
    if (q_out) SGD_HIP_TRY(hipMemcpyAsync(q_out, D.d_q, sizeof(double) * (size_t)P, hipMemcpyDeviceToHost, st));
    rc = D.wide_solve(io->l2, be, io->ridge != 0, io->fit_intercept != 0, io->max_sweeps, io->tol);
  } else {
    rc = D.inner_solve(io->l2, be, io->ridge != 0, io->fit_intercept != 0, io->max_sweeps, io->tol);
  }
  if (rc || (rc = fetch(io->cd_u, io->cd_a, io->cd_rec, 0, kRecLen))) return rc;
  io->V = sums[0];
  io->R = sums[1];
  // the candidate again, blended with the iterate at the caller's t
  SGD_HIP_TRY(hipMemcpyAsync(D.d_cand, io->u, sizeof(double) * (size_t)P, hipMemcpyHostToDevice, st));
  if ((rc = D.publish(io->t)) || (rc = fetch(io->blend_u, io->blend_a, io->blend_rec, kRecHalfSq, 4))) return rc;
  return SGDNET_OK;
}

}  // namespace

int newton_probe(const NewtonProblem& pb, sgdnet_newton_probe* io) { return newton_probe_steps(pb, io, false, 0, nullptr, nullptr, nullptr); }

int wnewton_probe(const NewtonProblem& pb, sgdnet_wnewton_probe_io* io) {
  const int width = io->width != 0 ? io->width : wide_cd_width((int)std::min<int64_t>(pb.p, kWnewtonMaxFeatures));
  io->ld = (int)wide_leading_dim(pb.p + 1);
  return newton_probe_steps(pb, io, true, width, io->H, io->Hd, io->q);
}

namespace {

// the geometry of a call's jobs: a function of (n, p, the groups, the number of mixes) alone.  wide: the row chunks of a
// job are those wnewton_run chooses for n_t rows (wide_layout.hpp), else newton_run's (dense_rows_per_chunk)
struct CvGeometry {
  int pairs = 0, max_chunks = 0, max_state_blocks = 0;
  std::vector<CvJob> jobs;
  CvGeometry(int64_t p, bool sparse, const int64_t* n_t, int n_sets, int n_mix, bool wide = false) {
    const int nc = (int)p + 2, T = (nc + kTileCols - 1) / kTileCols;
    pairs = T * (T + 1) / 2;
    jobs.resize((size_t)n_sets * (size_t)n_mix);
    for (int a = 0; a < n_mix; ++a)
      for (int t = 0; t < n_sets; ++t) {
        CvJob& J = jobs[(size_t)a * (size_t)n_sets + (size_t)t];
        J = CvJob{};
        J.n_t = n_t[t];
        J.set = t;
        J.rows_per_chunk = wide ? wide_rows_per_chunk(J.n_t, nc, kTileRows) : dense_rows_per_chunk(J.n_t, pairs);
        J.chunks = sparse ? 0 : (int32_t)((J.n_t + J.rows_per_chunk - 1) / J.rows_per_chunk);
        J.state_blocks = (int32_t)std::min<int64_t>(kStateMaxBlocks, (J.n_t + kBlock - 1) / kBlock);
        max_chunks = std::max(max_chunks, (int)J.chunks);
        max_state_blocks = std::max(max_state_blocks, (int)J.state_blocks);
      }
  }
  // per job: v, r, the moments and the chunks' partial tiles
  size_t workspace_doubles(int64_t n, int64_t p) const {
    return jobs.size() * (2 * (size_t)n + (size_t)(p + 2) * (size_t)(p + 2) + (size_t)max_chunks * (size_t)pairs * kBlock);
  }
};

}  // namespace

size_t newton_cv_workspace_bytes(int64_t n, int64_t p, bool sparse, const int64_t* n_t, int n_sets, int n_mix) {
  return sizeof(double) * CvGeometry(p, sparse, n_t, n_sets, n_mix).workspace_doubles(n, p);
}

size_t wnewton_cv_workspace_bytes(int64_t n, int64_t p, const int64_t* n_t, int n_sets, int n_mix, int n_lambda) {
  int64_t max_chunks = 0;
  for (int t = 0; t < n_sets; ++t) max_chunks = std::max(max_chunks, wnewton_row_chunks(n_t[t], p));
  return wnewton_cv_bytes((int64_t)n_sets * n_mix, n, p, n_lambda, max_chunks);
}

// The lock-step loop.  A round: the commands go up in one copy, every kernel is launched once over all jobs (a job whose
// command does not need a kernel leaves it at once), the records come back in one copy, and every job's state machine
// moves exactly as newton_run moves its one: a step is (moments, inner solve, state pass at the candidate); a candidate
// after which the objective rose is halved (blend, state pass) in the next round; an accepted candidate becomes the
// current iterate by flipping `cur`; a lambda that is done names the slot of U its iterate goes to.  The loop ends
// when every job has finished its last lambda; one last launch stores the iterates still owed.
// newton_cv_run and wnewton_cv_run: one loop, one state machine per job.  wide: the jobs' row chunks follow wide_row_chunks,
// newton_cv_wide_scale_kernel writes every stepping job's H, diag H and q to global memory, the inner solve is
// newton_cv_wide_cd_kernel<width> and the blend has no array of kNewtonMaxFeatures + 1.  Not wide: exactly the launches the
// Newton cross-validation has always made.
namespace {

static_assert(kTileRows == kWnewtonCvTileRows && kStateMaxBlocks == kWnewtonCvStateMaxBlocks && kRecLen == kWnewtonCvRecordDoubles &&
              kBlock == 256, "newton.hpp: wnewton_cv_bytes counts these");

int newton_cv_loop(const NewtonCvProblem& pb, bool timed, NewtonCvResult* out, bool wide, int width) {
  const int p = (int)pb.p, P = p + 1, nc = p + 2, L = pb.n_lambda, G = pb.n_sets;
  const int64_t n = pb.n;
  const bool sparse = pb.x_dense == nullptr;
  if (n <= 0 || pb.p <= 0 || pb.p > (wide ? kWnewtonMaxFeatures : kNewtonMaxFeatures) || L <= 0 || G <= 0 || pb.n_mix <= 0 || !pb.y ||
      !pb.start || !pb.mean || !pb.scale || !pb.b0 || !pb.l2 || !pb.l1 || !pb.ridge || pb.max_iter == 0 ||
      (sparse && (!pb.colptr || !pb.rowidx || !pb.values || !pb.cut)) || (int64_t)G * pb.n_mix > kNewtonCvMaxJobs ||
      (wide && (sparse || (width != kWideNarrow && width != kWideFull)))) {
    set_error("%s: invalid problem", wide ? "wnewton_cv_run" : "newton_cv_run");
    return SGDNET_EINVAL;
  }
  std::vector<int64_t> n_t((size_t)G);
  for (int t = 0; t < G; ++t) {
    const int64_t own = pb.start[t + 1] - pb.start[t];
    n_t[(size_t)t] = pb.train_on_rest ? n - own : own;
    if (own <= 0 || n_t[(size_t)t] <= 0) {
      set_error("%s: empty training set %d", wide ? "wnewton_cv_run" : "newton_cv_run", t);
      return SGDNET_EINVAL;
    }
  }
  CvGeometry geo(p, sparse, n_t.data(), G, pb.n_mix, wide);
  const int jobs = (int)geo.jobs.size(), ld = (int)wide_leading_dim(P);
  for (CvJob& J : geo.jobs) cv_job_rows(J, pb.start, n, pb.train_on_rest);
  const int64_t nnz = sparse ? pb.colptr[p] : 0;

  SGD_HIP_TRY(hipSetDevice(pb.device));
  Arena A;
  const size_t o_x = A.reserve(sizeof(double) * (size_t)(sparse ? nnz : n * (int64_t)p));
  const size_t o_colptr = A.reserve(sparse ? sizeof(int32_t) * (size_t)P : 0);
  const size_t o_rowidx = A.reserve(sparse ? sizeof(int32_t) * (size_t)nnz : 0);
  const size_t o_cut = A.reserve(sparse ? sizeof(int32_t) * (size_t)p * (size_t)(G + 1) : 0);
  const size_t o_y = A.reserve(sizeof(double) * (size_t)n);
  const size_t o_mu = A.reserve(sizeof(double) * (size_t)G * (size_t)p);
  const size_t o_scale = A.reserve(sizeof(double) * (size_t)G * (size_t)p);
  const size_t o_jobs = A.reserve(sizeof(CvJob) * (size_t)jobs);
  const size_t o_cmd = A.reserve(sizeof(CvCmd) * (size_t)jobs);
  const size_t o_v = A.reserve(sizeof(double) * (size_t)jobs * (size_t)n);
  const size_t o_r = A.reserve(sizeof(double) * (size_t)jobs * (size_t)n);
  const size_t o_part = A.reserve(sizeof(double) * (size_t)jobs * (size_t)geo.max_chunks * (size_t)geo.pairs * kBlock);
  const size_t o_M = A.reserve(sizeof(double) * (size_t)jobs * (size_t)nc * (size_t)nc);
  const size_t o_partial = A.reserve(sizeof(double) * (size_t)jobs * 3 * kStateMaxBlocks);
  const size_t o_sums = A.reserve(sizeof(double) * 2 * (size_t)jobs);
  const size_t o_rec = A.reserve(sizeof(double) * kRecLen * (size_t)jobs);
  const size_t o_u = A.reserve(sizeof(double) * 2 * (size_t)P * (size_t)jobs);
  const size_t o_a = A.reserve(sizeof(double) * (size_t)P * (size_t)jobs);
  const size_t o_U = A.reserve(sizeof(double) * (size_t)jobs * (size_t)L * (size_t)P);
  const size_t o_H = A.reserve(wide ? sizeof(double) * (size_t)jobs * (size_t)ld * (size_t)P : 0);
  const size_t o_Hd = A.reserve(wide ? sizeof(double) * (size_t)jobs * (size_t)P : 0);
  const size_t o_q = A.reserve(wide ? sizeof(double) * (size_t)jobs * (size_t)P : 0);
  SGD_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&A.base), A.used));
  double *d_H = A.at<double>(o_H), *d_Hd = A.at<double>(o_Hd), *d_q = A.at<double>(o_q);
  double *d_x = A.at<double>(o_x), *d_y = A.at<double>(o_y), *d_mu = A.at<double>(o_mu), *d_scale = A.at<double>(o_scale),
         *d_v = A.at<double>(o_v), *d_r = A.at<double>(o_r), *d_part = A.at<double>(o_part), *d_M = A.at<double>(o_M),
         *d_partial = A.at<double>(o_partial), *d_sums = A.at<double>(o_sums), *d_rec = A.at<double>(o_rec), *d_u = A.at<double>(o_u),
         *d_a = A.at<double>(o_a), *d_U = A.at<double>(o_U);
  int32_t *d_colptr = A.at<int32_t>(o_colptr), *d_rowidx = A.at<int32_t>(o_rowidx), *d_cut = A.at<int32_t>(o_cut);
  CvJob* d_jobs = A.at<CvJob>(o_jobs);
  CvCmd* d_cmd = A.at<CvCmd>(o_cmd);

  Stream sx;                           // (its rec_host is not used here: the records of all jobs come back into `pinned`)
  SGD_HIP_TRY(hipStreamCreateWithFlags(&sx.st, hipStreamNonBlocking));
  hipStream_t st = sx.st;
  if (timed)
    for (hipEvent_t& e : sx.e) SGD_HIP_TRY(hipEventCreate(&e));
  CvPinned pinned;                     // the commands of a round, then the records of its state passes
  SGD_HIP_TRY(hipHostMalloc(&pinned.p, sizeof(CvCmd) * (size_t)jobs + sizeof(double) * kRecLen * (size_t)jobs, hipHostMallocDefault));
  CvCmd* cmd = static_cast<CvCmd*>(pinned.p);
  const double* rec_all = reinterpret_cast<const double*>(cmd + jobs);

  // upload: x, y, the training sets' centres and scales, the jobs; both iterates of every job start at (0, b0)
  std::vector<double> start((size_t)jobs * 2 * (size_t)P, 0.0);
  for (int job = 0; job < jobs; ++job)
    for (int b = 0; b < 2; ++b) start[((size_t)job * 2 + (size_t)b) * (size_t)P + (size_t)p] = pb.b0[geo.jobs[(size_t)job].set];
  if (sparse) {
    if (nnz > 0) {
      SGD_HIP_TRY(hipMemcpyAsync(d_x, pb.values, sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice, st));
      SGD_HIP_TRY(hipMemcpyAsync(d_rowidx, pb.rowidx, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice, st));
    }
    SGD_HIP_TRY(hipMemcpyAsync(d_colptr, pb.colptr, sizeof(int32_t) * (size_t)P, hipMemcpyHostToDevice, st));
    SGD_HIP_TRY(hipMemcpyAsync(d_cut, pb.cut, sizeof(int32_t) * (size_t)p * (size_t)(G + 1), hipMemcpyHostToDevice, st));
    DeviceSetup& S = sx.S;             // the sample-major copy of the state pass (NewtonDevice::setup)
    S.n = n;
    S.p = p;
    S.nnz = nnz;
    if (nnz > 0) {
      S.colptr = d_colptr;
      S.rowidx = d_rowidx;
      S.val = d_x;
      const int rc = device_transpose(S, st);
      S.colptr = S.rowidx = nullptr;
      S.val = nullptr;
      if (rc) return rc;
    } else {
      SGD_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&S.sptr), sizeof(int64_t) * ((size_t)n + 1)));
      SGD_HIP_TRY(hipMemsetAsync(S.sptr, 0, sizeof(int64_t) * ((size_t)n + 1), st));
    }
  } else {
    SGD_HIP_TRY(hipMemcpyAsync(d_x, pb.x_dense, sizeof(double) * (size_t)(n * (int64_t)p), hipMemcpyHostToDevice, st));
  }
  SGD_HIP_TRY(hipMemcpyAsync(d_y, pb.y, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
  SGD_HIP_TRY(hipMemcpyAsync(d_mu, pb.mean, sizeof(double) * (size_t)G * (size_t)p, hipMemcpyHostToDevice, st));
  SGD_HIP_TRY(hipMemcpyAsync(d_scale, pb.scale, sizeof(double) * (size_t)G * (size_t)p, hipMemcpyHostToDevice, st));
  SGD_HIP_TRY(hipMemcpyAsync(d_jobs, geo.jobs.data(), sizeof(CvJob) * (size_t)jobs, hipMemcpyHostToDevice, st));
  SGD_HIP_TRY(hipMemcpyAsync(d_u, start.data(), sizeof(double) * start.size(), hipMemcpyHostToDevice, st));
  SGD_HIP_TRY(hipMemsetAsync(d_rec, 0, sizeof(double) * kRecLen * (size_t)jobs, st));

  out->loss.assign((size_t)jobs * (size_t)L, 0.0);
  out->unconverged.assign((size_t)jobs * (size_t)L, 0);
  out->passes.assign((size_t)jobs, 0.0);
  out->steps.assign((size_t)jobs, 0.0);
  out->halvings.assign((size_t)jobs, 0.0);
  out->sweeps = 0.0;
  out->rounds = 0;
  out->moments_ms = out->cd_ms = out->state_ms = out->scale_ms = 0.f;

  std::vector<CvJobState> state((size_t)jobs);
  const int centre = pb.centre ? 1 : 0, fit_intercept = pb.fit_intercept ? 1 : 0;
  auto penalties = [&](int job, int l, double* al, double* be) {
    const size_t at = (size_t)(job / G) * (size_t)L + (size_t)l;
    *al = pb.l2[at];
    *be = pb.ridge[job / G] ? 0.0 : pb.l1[at];
  };
  int live = jobs;
  for (;;) {
    bool any_step = false, any_blend = false;
    for (int job = 0; job < jobs; ++job) {
      const CvJobState& s = state[(size_t)job];
      cv_command(cmd[job], s, pb.ridge[job / G] != 0, [&](int l, double* al, double* be) { penalties(job, l, al, be); });
      any_step |= s.action == kCvStep;
      any_blend |= s.action == kCvHalve || s.action == kCvStart;
    }
    SGD_HIP_TRY(hipMemcpyAsync(d_cmd, cmd, sizeof(CvCmd) * (size_t)jobs, hipMemcpyHostToDevice, st));
    if (timed) SGD_HIP_TRY(hipEventRecord(sx.e[0], st));
    if (any_step) {
      if (sparse) {
        hipLaunchKernelGGL(newton_cv_sparse_pair_kernel, dim3((unsigned)p, (unsigned)nc, (unsigned)jobs), dim3(kBlock), 0, st, d_cmd, d_jobs,
                           d_cut, G, pb.train_on_rest ? 1 : 0, d_rowidx, d_x, d_v, d_r, d_mu, d_sums, n, p, d_M);
      } else {
        hipLaunchKernelGGL(newton_cv_dense_tile_kernel, dim3((unsigned)geo.pairs, (unsigned)geo.max_chunks, (unsigned)jobs), dim3(kBlock), 0,
                           st, d_cmd, d_jobs, d_x, d_v, d_r, d_mu, n, p, geo.max_chunks, d_part);
        hipLaunchKernelGGL(newton_cv_reduce_kernel, dim3((unsigned)geo.pairs, (unsigned)jobs), dim3(kBlock), 0, st, d_cmd, d_jobs, d_part,
                           geo.max_chunks, nc, d_M);
      }
    }
    if (timed) SGD_HIP_TRY(hipEventRecord(sx.e[1], st));
    // (the inner solve's kernel also stores the iterates owed to U: it runs in every round)
    if (wide) {
      if (any_step)
        hipLaunchKernelGGL(newton_cv_wide_scale_kernel, dim3((unsigned)P, (unsigned)jobs), dim3(kBlock), 0, st, d_cmd, d_jobs, d_M, d_scale,
                           p, ld, d_H, d_Hd, d_q);
      if (timed) SGD_HIP_TRY(hipEventRecord(sx.e[4], st));
      const auto kernel = width == kWideNarrow ? newton_cv_wide_cd_kernel<kWideNarrow> : newton_cv_wide_cd_kernel<kWideFull>;
      hipLaunchKernelGGL(kernel, dim3((unsigned)jobs), dim3((unsigned)width), 0, st, d_cmd, d_jobs, d_H, d_Hd, d_q, d_scale, p, ld, L,
                         fit_intercept, kNewtonMaxSweeps, pb.tol, d_u, d_a, d_rec, d_U);
      if (any_blend)
        hipLaunchKernelGGL(newton_cv_wide_blend_kernel, dim3((unsigned)jobs), dim3(64), 0, st, d_cmd, d_jobs, d_scale, p, d_u, d_a, d_rec);
    } else {
      hipLaunchKernelGGL(newton_cv_cd_kernel, dim3((unsigned)jobs), dim3(64), 0, st, d_cmd, d_jobs, d_M, d_scale, p, L, fit_intercept,
                         kNewtonMaxSweeps, pb.tol, d_u, d_a, d_rec, d_U);
      if (any_blend)
        hipLaunchKernelGGL(newton_cv_blend_kernel, dim3((unsigned)jobs), dim3(64), 0, st, d_cmd, d_jobs, d_scale, p, d_u, d_a, d_rec);
    }
    if (timed) SGD_HIP_TRY(hipEventRecord(sx.e[2], st));
    if (live > 0) {
      if (sparse)
        hipLaunchKernelGGL(newton_cv_state_kernel<true>, dim3((unsigned)geo.max_state_blocks, (unsigned)jobs), dim3(kBlock), 0, st, d_cmd,
                           d_jobs, sx.S.sval, sx.S.sptr, sx.S.sidx, d_y, d_mu, d_a, n, p, centre, d_v, d_r, d_partial);
      else
        hipLaunchKernelGGL(newton_cv_state_kernel<false>, dim3((unsigned)geo.max_state_blocks, (unsigned)jobs), dim3(kBlock), 0, st, d_cmd,
                           d_jobs, d_x, (const int64_t*)nullptr, (const int32_t*)nullptr, d_y, d_mu, d_a, n, p, 1, d_v, d_r, d_partial);
      hipLaunchKernelGGL(newton_cv_finish_kernel, dim3((unsigned)jobs), dim3(kBlock), 0, st, d_cmd, d_jobs, d_partial, d_sums, d_rec);
    }
    SGD_HIP_TRY(hipGetLastError());
    if (live == 0) break;              // (that was the launch that stores the last iterates)
    if (timed) SGD_HIP_TRY(hipEventRecord(sx.e[3], st));
    SGD_HIP_TRY(hipMemcpyAsync(const_cast<double*>(rec_all), d_rec, sizeof(double) * kRecLen * (size_t)jobs, hipMemcpyDeviceToHost, st));
    SGD_HIP_TRY(hipStreamSynchronize(st));
    ++out->rounds;
    if (timed) {
      float ms = 0.f;
      SGD_HIP_TRY(hipEventElapsedTime(&ms, sx.e[0], sx.e[1]));
      out->moments_ms += ms;
      if (wide) {
        SGD_HIP_TRY(hipEventElapsedTime(&ms, sx.e[1], sx.e[4]));
        out->scale_ms += ms;
      }
      SGD_HIP_TRY(hipEventElapsedTime(&ms, sx.e[wide ? 4 : 1], sx.e[2]));
      out->cd_ms += ms;
      SGD_HIP_TRY(hipEventElapsedTime(&ms, sx.e[2], sx.e[3]));
      out->state_ms += ms;
    }

    for (int job = 0; job < jobs; ++job)
      if (cv_job_advance(state[(size_t)job], rec_all + (size_t)job * kRecLen, L, pb.max_iter, pb.tol,
                         [&](int l, double* al, double* be) { penalties(job, l, al, be); }, out->loss.data() + (size_t)job * (size_t)L,
                         out->unconverged.data() + (size_t)job * (size_t)L, &out->passes[(size_t)job], &out->steps[(size_t)job],
                         &out->halvings[(size_t)job], &out->sweeps))
        --live;
  }
  out->u.resize((size_t)jobs * (size_t)L * (size_t)P);
  SGD_HIP_TRY(hipMemcpyAsync(out->u.data(), d_U, sizeof(double) * out->u.size(), hipMemcpyDeviceToHost, st));
  SGD_HIP_TRY(hipStreamSynchronize(st));
  return SGDNET_OK;
}

}  // namespace

int newton_cv_run(const NewtonCvProblem& pb, bool timed, NewtonCvResult* out) { return newton_cv_loop(pb, timed, out, false, 0); }

int wnewton_cv_run(const NewtonCvProblem& pb, bool timed, NewtonCvResult* out, int width) {
  return newton_cv_loop(pb, timed, out, true, width != 0 ? width : wide_cd_width((int)std::min<int64_t>(pb.p, kWnewtonMaxFeatures)));
}

}  // namespace sgdnet

extern "C" int sgdnet_newton_max_features(void) { return sgdnet::kNewtonMaxFeatures; }
extern "C" int sgdnet_wnewton_max_features(void) { return sgdnet::kWnewtonMaxFeatures; }
