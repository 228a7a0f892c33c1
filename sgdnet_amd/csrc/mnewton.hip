// Multinomial Newton mode (SGDNET_MODE_MNEWTON): the multinomial elastic-net path by proximal Newton steps on the JOINT
// Hessian of all classes.
//
// The problem is the one every mode fits (sgdnet_amd/kkt.py): features z_j = (x_j - m_j) / s_j, U = (w_k, b_k), k = 1 .. K,
//     F(U) = (1/n) sum_i [log sum_k e^eta_ik - eta_{i, y_i}] + sum_k (alpha/2 |w_k|^2 + beta |w_k|_1),   eta_ik = b_k + z_i'w_k,
// the b_k unpenalised (or frozen at the null model's values), alpha and beta the driver's (regularization_path).  The loss
// is flat along "the same shift for every class": the intercepts are defined up to a constant (the driver returns them
// with their class mean removed), and with alpha = 0 so are the coefficients of a feature no class of which is at zero
// -- at an even K the lasso optimum need not be unique.  Coordinate (k, j) lives at k P + j, P = p + 1, j = p the
// intercept; Q = K P.  One outer step from the iterate U0, warm-started lambda to lambda, as newton.hip takes it:
//
//   state      mnewton_state_kernel: eta_ik for all classes, the softmax with the row maximum subtracted (exp / log are
//              the plain-IEEE ones of include/sgdnet_detmath.h), mu (n x K, a column per class) and the loss, a thread
//              per sample.  Deviations are formed BEFORE they are multiplied: (x_ij - m_j) (w_kj / s_j).
//              mnewton_finish_kernel adds the workgroups' sums of the loss in workgroup order.
//   moments    with z~ = [x - m | 1], for every class pair k <= l
//                  H_kl = (1/n) sum_i mu_ik (delta_kl - mu_il) z~_i z~_i',      q_k = (1/n) sum_i (y_ik - mu_ik) z~_i
//              (f64; the 1/n and the driver's s_j are applied when the inner solve loads them): K (K + 1) / 2 weighted Gram
//              matrices of the same rows.  mnewton_pair_tile_kernel is newton_cv_dense_tile_kernel with the class pair
//              where that kernel has the job: the pair's weight is formed at staging from the stored mu, the q column is
//              staged as y_ik - mu_ik for the diagonal pairs (0 elsewhere); mnewton_pair_reduce_kernel adds the row
//              chunks in chunk order into one (p + 2)^2 matrix per pair.
//   inner      mnewton_cd_kernel: ONE workgroup keeps the packed triangle of the Q x Q joint Hessian, U and
//              g = H (U - U0) - q in LDS (mnewton.hpp: the budget behind sgdnet_mnewton_max_features) and runs
//              newton_cd_kernel's cyclic coordinate descent over all Q coordinates; the K intercepts have no penalty and
//              no threshold (a frozen intercept is never visited).  A coordinate whose diagonal entry is not positive
//              and that has no ridge term stays where it is.
//   accept     the state pass at the candidate gives its objective; the host halves a step after which it rose
//              (mnewton_blend_kernel), at most kNewtonMaxHalvings times.  The accepted candidate's pass is the next step's.
//
// Wide multinomial Newton mode (SGDNET_MODE_WMNEWTON, wmnewton_run) is the same outer loop for Q up to 5820 (mnewton.hpp):
// the state and moments passes as they are (the row chunks by wmnewton_row_chunks), then mnewton_wide_scale_kernel writes
// the full symmetric H, diag H and q to global memory and mnewton_wide_cd_kernel runs the shared wide descent core
// (wide_cd_device.hpp) over the Q coordinates; the blend forms its value where it is read (mnewton_wide_blend_kernel).
// Same optimum as the narrow mode, not the same bits; neither falls back to the other.
//
// Cross-validation (mnewton_cv_run, include/sgdnet_hip.h: sgdnet_cv_mnewton_*): all fold fits of all mixes advance in
// lock-step, as newton.hip's newton_cv_run runs the binomial ones.  The rows are sorted by group once, so a training set is
// a range of rows or the complement of one; the mnewton_cv_* kernels are the narrow mode's kernels with a job dimension,
// each job on its own rows, centres, scales and buffers (mu by the job's local row; (job, class pair) in one grid
// dimension of the moments pass); the command, the job and the host's state machine per job are newton_cv_device.hpp's,
// shared with newton.hip.
//
// x is dense, column-major: this mode's p is at most 98, and the driver expands sparse x before anything is computed from
// it (driver.cpp: fit_sparse_impl), so that a sparse fit is the dense fit of the same matrix from the standard deviations
// and lambda_max on, bit for bit.  No floating-point atomic anywhere and every reduction in an order fixed by (n, p, K):
// the same input gives the same bits.
//
// sgdnet_mnewton_probe (include/sgdnet_hip.h; mnewton_probe below) runs one outer step through the host steps of
// MNewtonDevice and copies every pass's output back: tests/test_gpu_mnewton_passes.py checks the passes one by one.
#define SGDNET_DET_MATH
#include <algorithm>
#include <utility>
#include <vector>

#include "common.hpp"
#include "device_math.hpp"
#include "mnewton.hpp"
#include "moments_device.hpp"
#include "newton_cv_device.hpp"
#include "wide_cd_device.hpp"

namespace sgdnet {
namespace {

constexpr int kStateMaxBlocks = 1024;   // workgroups of the state pass: each leaves one sum

// (the record of a candidate, in device memory, read by the host after every state pass: newton_cv_device.hpp)

// a[k P + j] = w_kj / s_j (j < p), a[k P + p] = b_k: the candidate as the state pass multiplies it.  mu[i + k n] holds
// eta_ik, then e^(eta_ik - max), then mu_ik.  Workgroup b leaves its sum of the loss in partial[b].
__global__ __launch_bounds__(kBlock) void mnewton_state_kernel(const double* __restrict__ x, const double* __restrict__ y,
                                                                const double* __restrict__ m, const double* __restrict__ a, int64_t n, int p,
                                                                int K, double* __restrict__ mu, double* __restrict__ partial) {
  __shared__ double sh[kBlock];
  const int P = p + 1;
  double loss = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const int yi = (int)(y[i] + 0.5);
    double mx = 0.0, eta_y = 0.0;
    for (int k = 0; k < K; ++k) {
      const double* __restrict__ ak = a + (size_t)k * (size_t)P;
      double eta = 0.0;
      for (int j = 0; j < p; ++j) eta += (x[i + (int64_t)j * n] - m[j]) * ak[j];
      eta += ak[p];
      mu[i + (int64_t)k * n] = eta;
      mx = k == 0 ? eta : fmax(mx, eta);
      if (k == yi) eta_y = eta;
    }
    double s = 0.0;
    for (int k = 0; k < K; ++k) {
      const double e = SGD_EXP(mu[i + (int64_t)k * n] - mx);
      mu[i + (int64_t)k * n] = e;
      s += e;
    }
    for (int k = 0; k < K; ++k) mu[i + (int64_t)k * n] /= s;
    loss += (SGD_LOG(s) + mx) - eta_y;
  }
  loss = block_sum(loss, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = loss;
}

// one workgroup: the sums of the state pass added in workgroup order; rec gets the mean loss
__global__ __launch_bounds__(kBlock) void mnewton_finish_kernel(const double* __restrict__ partial, int blocks, int64_t n,
                                                                 double* __restrict__ rec) {
  __shared__ double sh[kBlock];
  double s = 0.0;
  for (int b = threadIdx.x; b < blocks; b += kBlock) s += partial[b];
  s = block_sum(s, sh);
  if (threadIdx.x == 0) rec[kRecLoss] = s / (double)n;
}

// class pair c = 0 .. K (K + 1) / 2 - 1 -> (k, l), k <= l, row by row of the upper triangle
__device__ __forceinline__ void class_pair(int c, int K, int* k, int* l) {
  int kk = 0;
  while (c >= K - kk) {
    c -= K - kk;
    ++kk;
  }
  *k = kk;
  *l = kk + c;
}
__device__ __forceinline__ int class_pair_index(int k, int l, int K) { return k * K - k * (k - 1) / 2 + (l - k); }

// newton_cv_dense_tile_kernel with the class pair blockIdx.z where that kernel has the job: entry (a, b), a <= b, of the
// pair's (p + 2)^2 matrix is sum_i A_ia B_ib with A = [x - m | 1 | 0] and B = [v (x - m) | v | r], v_i = mu_ik (delta_kl -
// mu_il) and r_i = y_ik - mu_ik on the diagonal pairs, 0 elsewhere.  part[pair][chunk][tile pair][tid].
__global__ __launch_bounds__(kBlock) void mnewton_pair_tile_kernel(const double* __restrict__ x, const double* __restrict__ y,
                                                                    const double* __restrict__ mu, const double* __restrict__ m, int64_t n,
                                                                    int p, int K, int64_t rows_per_chunk, double* __restrict__ part) {
  __shared__ double A[kTileCols][kTileRows + 1], B[kTileCols][kTileRows + 1];
  const int tid = threadIdx.x, ncols = p + 2;
  const int T = (ncols + kTileCols - 1) / kTileCols;
  int pair = blockIdx.x, tj = 0;
  while (pair >= T - tj) {
    pair -= T - tj;
    ++tj;
  }
  const int tk = tj + pair;
  int ck, cl;
  class_pair((int)blockIdx.z, K, &ck, &cl);
  const double* __restrict__ mu_k = mu + (int64_t)ck * n;
  const double* __restrict__ mu_l = mu + (int64_t)cl * n;
  const int ta = tid & (kTileCols - 1), tb = tid / kTileCols;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_chunk;
  const int64_t r1 = r0 + rows_per_chunk < n ? r0 + rows_per_chunk : n;
  double acc = 0.0;
  for (int64_t base = r0; base < r1; base += kTileRows) {
    for (int e = tid; e < kTileCols * kTileRows; e += kBlock) {
      const int row = e & (kTileRows - 1), col = e / kTileRows;
      const int64_t i = base + row;
      const int ca = tj * kTileCols + col, cb = tk * kTileCols + col;
      double da = 0.0, db = 0.0;
      if (i < r1) {
        if (ca <= p) da = ca < p ? x[i + (int64_t)ca * n] - m[ca] : 1.0;
        if (cb == p + 1) {
          if (ck == cl) db = ((int)(y[i] + 0.5) == ck ? 1.0 : 0.0) - mu_k[i];
        } else if (cb <= p) {
          const double v = ck == cl ? mu_k[i] * (1.0 - mu_k[i]) : -(mu_k[i] * mu_l[i]);
          db = v * (cb < p ? x[i + (int64_t)cb * n] - m[cb] : 1.0);
        }
      }
      A[col][row] = da;
      B[col][row] = db;
    }
    __syncthreads();
    for (int i = 0; i < kTileRows; ++i) acc += A[ta][i] * B[tb][i];
    __syncthreads();
  }
  part[(((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * kBlock + tid] = acc;
}

// newton_cv_reduce_kernel for the class pair blockIdx.y: its chunks added in chunk order into M[pair]
__global__ __launch_bounds__(kBlock) void mnewton_pair_reduce_kernel(const double* __restrict__ part, int chunks, int ncols,
                                                                      double* __restrict__ M_all) {
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
  double* __restrict__ M = M_all + (size_t)blockIdx.y * (size_t)ncols * (size_t)ncols;
  double s = 0.0;
  for (int c = 0; c < chunks; ++c) s += part[(((size_t)blockIdx.y * (size_t)chunks + c) * gridDim.x + blockIdx.x) * kBlock + tid];
  M[(size_t)a * ncols + b] = s;
  if (tj != tk) M[(size_t)b * ncols + a] = s;
}

// What a candidate un[0 .. Q) leaves behind, by the workgroup's first wavefront (publish_candidate of newton.hip over K
// classes): itself and its state-pass form in memory, and in the record its penalty terms sum_k |w_k|^2 / 2 and
// sum_k |w_k|_1, its distance from the iterate max|un - u_cur| and its size max|un|.  Lane l takes the coordinates
// l, l + 64, ... in order; the lanes are joined by a butterfly.  Whatever the workgroup's width: the same bits.
template <class UP>
__device__ __forceinline__ void mnewton_publish(UP un, const double* __restrict__ u_cur, const double* __restrict__ scale, int p, int Q,
                                                double* __restrict__ u_cand, double* __restrict__ a_cand, double* __restrict__ rec) {
  const int lane = threadIdx.x, P = p + 1;
  if (lane >= 64) return;
  double sq = 0.0, ab = 0.0, ch = 0.0, sz = 0.0;
  for (int c = lane; c < Q; c += 64) {
    const int j = c % P;
    const double uc = un[c];
    ch = fmax(ch, fabs(uc - u_cur[c]));
    sz = fmax(sz, fabs(uc));
    if (j < p) {
      sq += uc * uc;
      ab += fabs(uc);
    }
    u_cand[c] = uc;
    a_cand[c] = j < p ? uc / scale[j] : uc;
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
__global__ __launch_bounds__(64) void mnewton_blend_kernel(const double* __restrict__ u_cur, const double* __restrict__ scale, int p, int Q,
                                                            double t, double* __restrict__ u_cand, double* __restrict__ a_cand,
                                                            double* __restrict__ rec) {
  __shared__ double un[kMNewtonMaxCoordinates];
  for (int c = threadIdx.x; c < Q; c += 64) un[c] = t == 1.0 ? u_cand[c] : u_cur[c] + t * (u_cand[c] - u_cur[c]);
  __syncthreads();
  mnewton_publish(un, u_cur, scale, p, Q, u_cand, a_cand, rec);
}

// One workgroup of kWidth lanes, one inner solve.  Every lane computes the sweep's scalars (the new coordinate, the
// sweep's max|du| and max|u|) from the same LDS words, so branches on them are uniform and nothing has to be broadcast
// (newton_cd_kernel); the width only spreads the update of g, an entry per lane, so both widths give the same bits.
// M: the K (K + 1) / 2 pair moments, (p + 2)^2 each (upper triangle), dn = n; the quadratic model about u_cur is
//   (U - U0)'H (U - U0) / 2 - q'(U - U0) + sum_k (al/2 |w_k|^2 + be |w_k|_1),     its smooth gradient g = H (U - U0) - q.
// (the body of mnewton_cd_kernel and of mnewton_cv_cd_kernel, which runs it once per job; lds: the workgroup's whole LDS)
template <int kWidth>
__device__ __forceinline__ void mnewton_cd_solve(double* lds, const double* __restrict__ M, const double* __restrict__ scale, int p, int K,
                                                 double dn, const double* __restrict__ u_cur, double al, double be, int ridge,
                                                 int fit_intercept, unsigned max_sweeps, double tol, double* __restrict__ u_cand,
                                                 double* __restrict__ a_cand, double* __restrict__ rec) {
  const int lane = threadIdx.x, P = p + 1, nc = p + 2, Q = K * P;
  const size_t block = (size_t)nc * (size_t)nc;
  double* H = lds;
  double* u = H + Q * (Q + 1) / 2;
  double* g = u + Q;
  for (int c2 = 0; c2 < Q; ++c2) {
    const int l = c2 / P, b = c2 - l * P;
    const double sb = b < p ? scale[b] : 1.0;
    for (int c1 = lane; c1 <= c2; c1 += kWidth) {
      const int k = c1 / P, a = c1 - k * P;         // k <= l
      const int lo = a < b ? a : b, hi = a < b ? b : a;
      H[tri(c1, c2)] = M[(size_t)class_pair_index(k, l, K) * block + (size_t)lo * nc + hi] / dn / ((a < p ? scale[a] : 1.0) * sb);
    }
  }
  for (int c = lane; c < Q; c += kWidth) {
    const int k = c / P, a = c - k * P;
    g[c] = -(M[(size_t)class_pair_index(k, k, K) * block + (size_t)a * nc + p + 1] / dn / (a < p ? scale[a] : 1.0));
    u[c] = u_cur[c];
  }
  __syncthreads();
  unsigned sweeps = 0;
  bool converged = false, negligible = false;
  while (sweeps < max_sweeps && !converged) {
    double max_change = 0.0, max_size = 0.0, max_eta_sq = 0.0;
    for (int k = 0, j = 0; k < K; ++k) {
      for (int a = 0; a < P; ++a, ++j) {
        const bool penalised = a < p;
        if (!penalised && !fit_intercept) continue;          // (the frozen intercept is never visited: it stays at u_cur)
        const double uj = u[j], hjj = H[tri(j, j)];
        const double z = hjj * uj - g[j], denom = penalised ? hjj + al : hjj;
        double nu = z;
        if (penalised && !ridge) nu = z > be ? z - be : (z < -be ? z + be : 0.0);
        // a constant column without an l2 term: H_jj = q_j = 0; every weight underflowed: the coordinate stays
        nu = denom > 0.0 ? nu / denom : uj;
        // what the threshold leaves of a coordinate when |z| equals it but for rounding (lambda_max: newton.hpp,
        // kNewtonNegligible) is an exact zero: a path that starts at lambda_max starts with all coefficients 0.0.
        // (Not for a coordinate that stays: with H_jj = 0 the test holds whatever uj is.)
        if (penalised && !ridge && denom > 0.0 && nu * nu * hjj <= kNewtonNegligible * kNewtonNegligible) nu = 0.0;
        const double d = nu - uj;
        max_change = fmax(max_change, fabs(d));
        max_size = fmax(max_size, fabs(nu));
        max_eta_sq = fmax(max_eta_sq, nu * nu * hjj);
        if (d != 0.0) {
          __syncthreads();                         // every lane has read u[j] and g[j]
          if (lane == 0) u[j] = nu;
          for (int c = lane; c < Q; c += kWidth) g[c] += H[c <= j ? tri(c, j) : tri(j, c)] * d;
          __syncthreads();
        }
      }
    }
    ++sweeps;
    const bool all_zero = max_size == 0.0 && max_change == 0.0;
    const bool no_change = max_size != 0.0 && max_change / max_size <= tol;
    negligible = max_eta_sq <= kNewtonNegligible * kNewtonNegligible;      // zero to rounding (newton.hpp)
    converged = all_zero || no_change || negligible;
  }
  __syncthreads();
  mnewton_publish(u, u_cur, scale, p, Q, u_cand, a_cand, rec);
  if (lane == 0) {
    rec[kRecSweeps] = (double)sweeps;
    rec[kRecInnerConverged] = converged ? 1.0 : 0.0;
    rec[kRecNegligible] = negligible ? 1.0 : 0.0;
  }
}

template <int kWidth>
__global__ __launch_bounds__(kWidth) void mnewton_cd_kernel(const double* __restrict__ M, const double* __restrict__ scale, int p, int K,
                                                             double dn, const double* __restrict__ u_cur, double al, double be, int ridge,
                                                             int fit_intercept, unsigned max_sweeps, double tol, double* __restrict__ u_cand,
                                                             double* __restrict__ a_cand, double* __restrict__ rec) {
  __shared__ double lds[mnewton_state_doubles(kMNewtonMaxCoordinates)];
  mnewton_cd_solve<kWidth>(lds, M, scale, p, K, dn, u_cur, al, be, ridge, fit_intercept, max_sweeps, tol, u_cand, a_cand, rec);
}

// One wavefront while one stride of it covers the coordinates; 256 lanes beyond (profiles/mnewton_path.txt).
int mnewton_cd_width(int Q) { return Q <= 64 ? 64 : 256; }

// ---- cross-validation (mnewton_cv_run): the kernels above with a job dimension ----
// A job is one (mix, training set), its command, its rows (cv_row) and its record as newton_cv_device.hpp has them: shared
// with newton.hip's cross-validation.  Every job has its own a, mu, sums, pair moments, record, two iterates and slice of
// U; its centres and scales are its training set's; its grids (state workgroups, row chunks, the inner solve's width) are
// those mnewton_run would choose for n_t rows, so its arithmetic is the same whichever other jobs share the launch.
// mu of a job is indexed by the job's LOCAL row li = 0 .. n_t - 1, a column per class, from mu_at[job] on.

// mnewton_state_kernel for the job blockIdx.y over the job's rows; workgroup b of the job leaves its sum in partial[job][b]
__global__ __launch_bounds__(kBlock) void mnewton_cv_state_kernel(const CvCmd* __restrict__ cmd, const CvJob* __restrict__ jobs,
                                                                   const int64_t* __restrict__ mu_at, const double* __restrict__ x,
                                                                   const double* __restrict__ y, const double* __restrict__ m_all,
                                                                   const double* __restrict__ a_all, int64_t n, int p, int K,
                                                                   double* __restrict__ mu_all, double* __restrict__ partial_all) {
  __shared__ double sh[kBlock];
  const int job = blockIdx.y;
  if (cmd[job].action == kCvIdle) return;
  const CvJob J = jobs[job];
  if ((int)blockIdx.x >= J.state_blocks) return;
  const int P = p + 1;
  const int64_t nt = J.n_t;
  const double* __restrict__ m = m_all + (size_t)J.set * (size_t)p;
  const double* __restrict__ a = a_all + (size_t)job * (size_t)K * (size_t)P;
  double* __restrict__ mu = mu_all + mu_at[job];
  double loss = 0.0;
  for (int64_t li = (int64_t)blockIdx.x * kBlock + threadIdx.x; li < nt; li += (int64_t)J.state_blocks * kBlock) {
    const int64_t i = cv_row(J, li);
    const int yi = (int)(y[i] + 0.5);
    double mx = 0.0, eta_y = 0.0;
    for (int k = 0; k < K; ++k) {
      const double* __restrict__ ak = a + (size_t)k * (size_t)P;
      double eta = 0.0;
      for (int j = 0; j < p; ++j) eta += (x[i + (int64_t)j * n] - m[j]) * ak[j];
      eta += ak[p];
      mu[li + (int64_t)k * nt] = eta;
      mx = k == 0 ? eta : fmax(mx, eta);
      if (k == yi) eta_y = eta;
    }
    double s = 0.0;
    for (int k = 0; k < K; ++k) {
      const double e = SGD_EXP(mu[li + (int64_t)k * nt] - mx);
      mu[li + (int64_t)k * nt] = e;
      s += e;
    }
    for (int k = 0; k < K; ++k) mu[li + (int64_t)k * nt] /= s;
    loss += (SGD_LOG(s) + mx) - eta_y;
  }
  loss = block_sum(loss, sh);
  if (threadIdx.x == 0) partial_all[(size_t)job * kStateMaxBlocks + blockIdx.x] = loss;
}

// mnewton_finish_kernel for the job blockIdx.x: the mean is over the job's n_t rows
__global__ __launch_bounds__(kBlock) void mnewton_cv_finish_kernel(const CvCmd* __restrict__ cmd, const CvJob* __restrict__ jobs,
                                                                    const double* __restrict__ partial_all, double* __restrict__ rec_all) {
  __shared__ double sh[kBlock];
  const int job = blockIdx.x;
  if (cmd[job].action == kCvIdle) return;
  const double* __restrict__ partial = partial_all + (size_t)job * kStateMaxBlocks;
  const int blocks = jobs[job].state_blocks;
  double s = 0.0;
  for (int b = threadIdx.x; b < blocks; b += kBlock) s += partial[b];
  s = block_sum(s, sh);
  if (threadIdx.x == 0) rec_all[(size_t)job * kRecLen + kRecLoss] = s / (double)jobs[job].n_t;
}

// mnewton_pair_tile_kernel with (job, class pair) = blockIdx.z / class pairs, blockIdx.z % class pairs: blockIdx.y is a chunk
// of the JOB's rows.  part[job][pair][chunk <= max_chunks][tile pair][tid].
__global__ __launch_bounds__(kBlock) void mnewton_cv_pair_tile_kernel(const CvCmd* __restrict__ cmd, const CvJob* __restrict__ jobs,
                                                                       const int64_t* __restrict__ mu_at, const double* __restrict__ x,
                                                                       const double* __restrict__ y, const double* __restrict__ mu_all,
                                                                       const double* __restrict__ m_all, int64_t n, int p, int K,
                                                                       int max_chunks, double* __restrict__ part) {
  __shared__ double A[kTileCols][kTileRows + 1], B[kTileCols][kTileRows + 1];
  const int class_pairs = K * (K + 1) / 2;
  const int job = (int)blockIdx.z / class_pairs, cp = (int)blockIdx.z - job * class_pairs;
  if (cmd[job].action != kCvStep) return;
  const CvJob J = jobs[job];
  if ((int)blockIdx.y >= J.chunks) return;
  const double* __restrict__ m = m_all + (size_t)J.set * (size_t)p;
  const int tid = threadIdx.x, ncols = p + 2;
  const int T = (ncols + kTileCols - 1) / kTileCols;
  int pair = blockIdx.x, tj = 0;
  while (pair >= T - tj) {
    pair -= T - tj;
    ++tj;
  }
  const int tk = tj + pair;
  int ck, cl;
  class_pair(cp, K, &ck, &cl);
  const double* __restrict__ mu_k = mu_all + mu_at[job] + (int64_t)ck * J.n_t;
  const double* __restrict__ mu_l = mu_all + mu_at[job] + (int64_t)cl * J.n_t;
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
        if (ca <= p) da = ca < p ? x[i + (int64_t)ca * n] - m[ca] : 1.0;
        if (cb == p + 1) {
          if (ck == cl) db = ((int)(y[i] + 0.5) == ck ? 1.0 : 0.0) - mu_k[li];
        } else if (cb <= p) {
          const double v = ck == cl ? mu_k[li] * (1.0 - mu_k[li]) : -(mu_k[li] * mu_l[li]);
          db = v * (cb < p ? x[i + (int64_t)cb * n] - m[cb] : 1.0);
        }
      }
      A[col][row] = da;
      B[col][row] = db;
    }
    __syncthreads();
    for (int i = 0; i < kTileRows; ++i) acc += A[ta][i] * B[tb][i];
    __syncthreads();
  }
  part[(((size_t)blockIdx.z * (size_t)max_chunks + blockIdx.y) * gridDim.x + blockIdx.x) * kBlock + tid] = acc;
}

// mnewton_pair_reduce_kernel for (job, class pair) = blockIdx.y: the job's chunks added in chunk order into M[job][pair]
__global__ __launch_bounds__(kBlock) void mnewton_cv_pair_reduce_kernel(const CvCmd* __restrict__ cmd, const CvJob* __restrict__ jobs,
                                                                         const double* __restrict__ part, int class_pairs, int max_chunks,
                                                                         int ncols, double* __restrict__ M_all) {
  const int job = (int)blockIdx.y / class_pairs;
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
  double* __restrict__ M = M_all + (size_t)blockIdx.y * (size_t)ncols * (size_t)ncols;
  double s = 0.0;
  for (int c = 0; c < chunks; ++c) s += part[(((size_t)blockIdx.y * (size_t)max_chunks + c) * gridDim.x + blockIdx.x) * kBlock + tid];
  M[(size_t)a * ncols + b] = s;
  if (tj != tk) M[(size_t)b * ncols + a] = s;
}

// mnewton_blend_kernel for the job blockIdx.x: a halving (t = 1/2), or the path's start published as it is (t = 1)
__global__ __launch_bounds__(64) void mnewton_cv_blend_kernel(const CvCmd* __restrict__ cmd, const CvJob* __restrict__ jobs,
                                                               const double* __restrict__ scale_all, int p, int Q, double* __restrict__ u_all,
                                                               double* __restrict__ a_all, double* __restrict__ rec_all) {
  __shared__ double un[kMNewtonMaxCoordinates];
  const int job = blockIdx.x;
  const CvCmd c = cmd[job];
  if (c.action != kCvHalve && c.action != kCvStart) return;
  const double* __restrict__ u_cur = u_all + ((size_t)job * 2 + (size_t)c.cur) * (size_t)Q;
  double* __restrict__ u_cand = u_all + ((size_t)job * 2 + (size_t)(1 - c.cur)) * (size_t)Q;
  const double t = c.action == kCvStart ? 1.0 : 0.5;
  for (int k = threadIdx.x; k < Q; k += 64) un[k] = t == 1.0 ? u_cand[k] : u_cur[k] + t * (u_cand[k] - u_cur[k]);
  __syncthreads();
  mnewton_publish(un, u_cur, scale_all + (size_t)jobs[job].set * (size_t)p, p, Q, u_cand, a_all + (size_t)job * (size_t)Q,
                  rec_all + (size_t)job * kRecLen);
}

// mnewton_cd_kernel for the job blockIdx.x: one workgroup per job, each declaring the whole LDS, so the jobs spread one
// per CU.  Before anything else it stores the current iterate into U[slot] where the host says it answers a lambda.
template <int kWidth>
__global__ __launch_bounds__(kWidth) void mnewton_cv_cd_kernel(const CvCmd* __restrict__ cmd, const CvJob* __restrict__ jobs,
                                                                const double* __restrict__ M_all, const double* __restrict__ scale_all, int p,
                                                                int K, int n_lambda, int fit_intercept, unsigned max_sweeps, double tol,
                                                                double* __restrict__ u_all, double* __restrict__ a_all,
                                                                double* __restrict__ rec_all, double* __restrict__ U_all) {
  __shared__ double lds[mnewton_state_doubles(kMNewtonMaxCoordinates)];
  const int job = blockIdx.x, nc = p + 2, Q = K * (p + 1), class_pairs = K * (K + 1) / 2;
  const CvCmd c = cmd[job];
  const double* __restrict__ u_cur = u_all + ((size_t)job * 2 + (size_t)c.cur) * (size_t)Q;
  if (c.slot >= 0) {
    double* __restrict__ U = U_all + ((size_t)job * (size_t)n_lambda + (size_t)c.slot) * (size_t)Q;
    for (int k = threadIdx.x; k < Q; k += kWidth) U[k] = u_cur[k];
  }
  if (c.action != kCvStep) return;
  mnewton_cd_solve<kWidth>(lds, M_all + (size_t)job * (size_t)class_pairs * (size_t)nc * (size_t)nc,
                           scale_all + (size_t)jobs[job].set * (size_t)p, p, K, (double)jobs[job].n_t, u_cur, c.l2, c.l1, c.ridge,
                           fit_intercept, max_sweeps, tol, u_all + ((size_t)job * 2 + (size_t)(1 - c.cur)) * (size_t)Q,
                           a_all + (size_t)job * (size_t)Q, rec_all + (size_t)job * kRecLen);
}

// ---- wide multinomial Newton mode (SGDNET_MODE_WMNEWTON, wmnewton_run): H in global memory, only what can move is touched ----

// mnewton_blend_kernel without an array of kMNewtonMaxCoordinates doubles: mnewton_publish reads every coordinate once, by
// the lane that then writes it, so the blend is formed where it is read (newton.hip: BlendedCandidate).
struct BlendedCandidate {
  const double* u_cur;
  const double* u_cand;
  double t;
  __device__ __forceinline__ double operator[](int c) const { return t == 1.0 ? u_cand[c] : u_cur[c] + t * (u_cand[c] - u_cur[c]); }
};

__global__ __launch_bounds__(64) void mnewton_wide_blend_kernel(const double* u_cur, const double* __restrict__ scale, int p, int Q, double t,
                                                                 double* u_cand, double* __restrict__ a_cand, double* __restrict__ rec) {
  mnewton_publish(BlendedCandidate{u_cur, u_cand, t}, u_cur, scale, p, Q, u_cand, a_cand, rec);
}

// blockIdx.x = column c2 of the joint Hessian over the Q = K P coordinates: H[c1 + ld c2] for all c1 < Q from the
// K (K + 1) / 2 pair moments with the arithmetic of mnewton_cd_kernel's prologue -- M[pair(k, l)][lo nc + hi] / dn / (s_a s_b),
// the class pair in ascending order on either side of the diagonal, s = scale for the p features and 1 for the intercepts --
// so an entry has the bits the narrow kernel would hold; rows Q .. ld - 1 are the zero pad.  Also diag H, and
// q[c2] = M[pair(l, l)][b nc + p + 1] / dn / s_b.
__global__ __launch_bounds__(kBlock) void mnewton_wide_scale_kernel(const double* __restrict__ M, const double* __restrict__ scale, int p, int K,
                                                                     int ld, double dn, double* __restrict__ H, double* __restrict__ Hd,
                                                                     double* __restrict__ q) {
  const int P = p + 1, nc = p + 2, Q = K * P;
  const size_t block = (size_t)nc * (size_t)nc;
  const int c2 = blockIdx.x, l = c2 / P, b = c2 - l * P;
  const double sb = b < p ? scale[b] : 1.0;
  for (int c1 = threadIdx.x; c1 < ld; c1 += kBlock) {
    double v = 0.0;
    if (c1 < Q) {
      const int k = c1 / P, a = c1 - k * P;
      const int lo = a < b ? a : b, hi = a < b ? b : a;
      const double sa = a < p ? scale[a] : 1.0;
      const int pair = k <= l ? class_pair_index(k, l, K) : class_pair_index(l, k, K);
      // (the narrow kernel multiplies the scale of the smaller coordinate by that of the larger; the product commutes)
      v = M[(size_t)pair * block + (size_t)lo * nc + hi] / dn / (sa * sb);
    }
    H[(size_t)c2 * ld + c1] = v;
    if (c1 == c2) Hd[c2] = v;
  }
  if (threadIdx.x == 0) q[c2] = M[(size_t)class_pair_index(l, l, K) * block + (size_t)b * nc + p + 1] / dn / sb;
}

// The coordinate update of mnewton_cd_kernel, for the screen (u_j = 0) and for the sweep: from H_jj, u_j and g_j to the new
// u_j.  Its two rules that newton_coord_new_u has not: a coordinate whose denominator is not positive stays where it is, and
// what the threshold leaves of a penalised coordinate when |z| equals it but for rounding is an exact zero (where the
// denominator is positive, and not under ridge).  Every caller passes the same words through the same operations, so every
// lane holds the same bits.
__device__ __forceinline__ double mnewton_coord_new_u(double hjj, double uj, double gj, double al, double be, int ridge, bool penalised) {
  const double z = hjj * uj - gj, denom = penalised ? hjj + al : hjj;
  double nu = z;
  if (penalised && !ridge) nu = z > be ? z - be : (z < -be ? z + be : 0.0);
  nu = denom > 0.0 ? nu / denom : uj;
  if (penalised && !ridge && denom > 0.0 && nu * nu * hjj <= kNewtonNegligible * kNewtonNegligible) nu = 0.0;
  return nu;
}

// One workgroup of kWidth lanes, one inner solve, H (leading dimension ld, a multiple of 16) read from global memory:
// newton_wide_cd_kernel over the Q joint coordinates.
// LDS (mnewton.hpp: wmnewton_state_bytes): g | U | diag H | the list | the list's bits | the compaction's counts.
//   start    U = U_cur, so g = H (U - U_cur) - q = -q exactly: no pass over H.  The list is {c : c mod P < p, U_c != 0} and
//            the K intercept coordinates c mod P == p when they are fitted (unpenalised, without threshold; frozen: never
//            visited).
//   screen   every penalised c outside the list: the coordinate update from U_c = 0; those that would move join.  The list
//            is compacted again in ascending order (wide_cd_device.hpp: wide_compact).
//   sweep    mnewton_cd_kernel's coordinate update over the list: every lane computes the scalars from the same LDS words
//            (uniform branches); a coordinate that stays costs no global read and no barrier; one that moves by d does
//            g[c'] += H[c', c] d for ALL c' < Q, 16 bytes a lane, so g stays the full gradient and the screen needs no pass
//            over H.  The sweeps end as mnewton_cd_kernel's do; then the screen runs again, and the solve is done when it
//            adds nothing.
// max_sweeps bounds the list sweeps of the solve.  g[c] is updated by one lane from the same words in the same order
// whatever kWidth is, and the candidate is published by the first wavefront alone: both widths give the same bits.
template <int kWidth>
__global__ __launch_bounds__(kWidth) void mnewton_wide_cd_kernel(const double* __restrict__ H, const double* __restrict__ Hd,
                                                                  const double* __restrict__ q, const double* __restrict__ scale, int p, int K,
                                                                  int ld, const double* __restrict__ u_cur, double al, double be, int ridge,
                                                                  int fit_intercept, unsigned max_sweeps, double tol,
                                                                  double* __restrict__ u_cand, double* __restrict__ a_cand,
                                                                  double* __restrict__ rec) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[kWmnewtonLdsBytes];
  const int lane = threadIdx.x, wave = lane >> 6, P = p + 1, Q = K * P;
  double* g = reinterpret_cast<double*>(lds);
  double* u = g + Q;
  double* hd = u + Q;
  int32_t* list = reinterpret_cast<int32_t*>(hd + Q);
  uint32_t* bits = reinterpret_cast<uint32_t*>(list + Q);
  int32_t* counts = reinterpret_cast<int32_t*>(bits + (Q + 31) / 32);
  for (int c = lane; c < Q; c += kWidth) {
    g[c] = -q[c];
    u[c] = u_cur[c];
    hd[c] = Hd[c];
  }
  __syncthreads();

  // The list from one flag per coordinate (wide_compact).  screen: the flag is "in the list already, or would move from 0";
  // else: the start's.  An intercept coordinate is in iff the intercepts are fitted.
  auto compact = [&](bool screen) -> int {
    return wide_compact<kWidth>(Q, list, bits, counts, [&](int c) -> bool {
      bool in = false;
      if (c < Q) {
        if (c % P < p) {
          if (screen) {
            in = (bits[c >> 5] >> (c & 31)) & 1u;
            if (!in) in = mnewton_coord_new_u(hd[c], 0.0, g[c], al, be, ridge, true) != 0.0;
          } else {
            in = u[c] != 0.0;
          }
        } else {
          in = fit_intercept != 0;
        }
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
        const int c = list[i];
        const double uj = u[c], hjj = hd[c];
        const double nu = mnewton_coord_new_u(hjj, uj, g[c], al, be, ridge, c % P < p);
        const double d = nu - uj;
        max_change = fmax(max_change, fabs(d));
        max_size = fmax(max_size, fabs(nu));
        max_eta_sq = fmax(max_eta_sq, nu * nu * hjj);
        if (d != 0.0) {
          __syncthreads();                         // every lane has read u[c] and g[c]
          if (lane == 0) u[c] = nu;
          wide_column_move<kWidth>(g, H + (size_t)ld * c, Q, d);
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
    mnewton_publish(u, u_cur, scale, p, Q, u_cand, a_cand, rec);
    if (lane == 0) {
      rec[kRecSweeps] = (double)sweeps;
      rec[kRecInnerConverged] = converged ? 1.0 : 0.0;
      rec[kRecNegligible] = negligible ? 1.0 : 0.0;
    }
  }
}

// The wide inner solve's workgroup.  Both instances give the same bits; profiles/wmnewton_path.txt has the inner solves'
// time per 100-lambda path (mix 0.5) at Q = K (p + 1) = 15, 198, 2010, 3003 and 5002:
//   lanes      Q = 15     198      2010     3003     5002
//   256        11.3 ms   89.4 ms   1442 ms  2931 ms  2353 ms
//   1024       14.7 ms   118 ms     679 ms  1851 ms  1240 ms
// Up to one stride of 256 lanes twelve more wavefronts only wait at the barriers; from 2000 coordinates on sixteen
// wavefronts take 0.47 to 0.63 of the time.  Nothing was measured between 198 and 2010, so wide_layout.hpp's rule over
// the Q coordinates (256 lanes up to 512, 1024 beyond), which both ends agree with, stands here too.
int wmnewton_cd_width(int Q) { return wide_cd_width(Q); }

struct Stream {
  hipStream_t st = nullptr;
  hipEvent_t e[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // (4: wide only, behind the scale kernel)
  double* rec_host = nullptr;          // pinned: the record of a state pass
  ~Stream() {
    for (hipEvent_t v : e)
      if (v) (void)hipEventDestroy(v);
    if (rec_host) (void)hipHostFree(rec_host);
    if (st) (void)hipStreamDestroy(st);
  }
};

// What one problem keeps on the device and the launches of an outer step as named host steps (NewtonDevice of newton.hip).
struct MNewtonDevice {
  int64_t n = 0;
  int p = 0, P = 0, nc = 0, K = 0, Q = 0, class_pairs = 0, width = 64;
  bool timed = false;
  // the wide mode (wmnewton_run; set before setup): H, diag H and q in global memory, the inner solve on `width` lanes
  // (256 or 1024), the row chunks of mnewton.hpp's wmnewton_row_chunks
  bool wide = false;
  int ld = 0;
  double *d_H = nullptr, *d_Hd = nullptr, *d_q = nullptr;
  int pairs = 0;                       // the tile pairs and the row chunks (a function of n, p and K alone)
  int64_t rows_per_chunk = 0, chunks = 0;
  int state_blocks = 0;
  Arena A;
  Stream sx;
  hipStream_t st = nullptr;
  double *d_x = nullptr, *d_y = nullptr, *d_mu = nullptr, *d_m = nullptr, *d_scale = nullptr, *d_part = nullptr, *d_M = nullptr,
         *d_partial = nullptr, *d_rec = nullptr, *d_a = nullptr, *d_cur = nullptr, *d_cand = nullptr, *d_U = nullptr;
  const double* rec = nullptr;         // the pinned copy of the record, as of the last state pass
  double passes = 0.0;
  float state_ms = 0.f;

  // u_cur: the iterate; u_cand: the candidate the first publish takes (a fit starts with both at the path's start)
  int setup(const MNewtonProblem& pb, const double* u_cur, const double* u_cand, bool timed_, int width_) {
    n = pb.n;
    p = (int)pb.p;
    P = p + 1;
    nc = p + 2;
    K = pb.K;
    Q = K * P;
    class_pairs = K * (K + 1) / 2;
    timed = timed_;
    if (wide) width = width_;            // (wmnewton_loop's caller has resolved and checked it)
    else width = width_ == 64 || width_ == 256 ? width_ : mnewton_cd_width(Q);
    const int L = pb.n_lambda;
    SGD_HIP_TRY(hipSetDevice(pb.device));
    const int T = (nc + kTileCols - 1) / kTileCols;
    pairs = T * (T + 1) / 2;
    // (the chunk count shrinks with all the workgroups of a chunk: tile pairs x class pairs)
    rows_per_chunk = wide ? wmnewton_rows_per_chunk(n, nc, K, kTileRows) : dense_rows_per_chunk(n, pairs * class_pairs);
    chunks = (n + rows_per_chunk - 1) / rows_per_chunk;
    ld = (int)wide_leading_dim(Q);
    state_blocks = (int)std::min<int64_t>(kStateMaxBlocks, (n + kBlock - 1) / kBlock);

    const size_t o_x = A.reserve(sizeof(double) * (size_t)(n * (int64_t)p));
    const size_t o_y = A.reserve(sizeof(double) * (size_t)n);
    const size_t o_mu = A.reserve(sizeof(double) * (size_t)n * (size_t)K);
    const size_t o_m = A.reserve(sizeof(double) * (size_t)nc);           // cov_sum_kernel: the means, then the sum and the mean of y
    const size_t o_scale = A.reserve(sizeof(double) * (size_t)p);
    const size_t o_part = A.reserve(sizeof(double) * (size_t)class_pairs * (size_t)chunks * (size_t)pairs * kBlock);
    const size_t o_M = A.reserve(sizeof(double) * (size_t)class_pairs * (size_t)nc * (size_t)nc);
    const size_t o_partial = A.reserve(sizeof(double) * (size_t)state_blocks);
    const size_t o_rec = A.reserve(sizeof(double) * kRecLen);
    const size_t o_u0 = A.reserve(sizeof(double) * (size_t)Q);
    const size_t o_u1 = A.reserve(sizeof(double) * (size_t)Q);
    const size_t o_a = A.reserve(sizeof(double) * (size_t)Q);
    const size_t o_U = A.reserve(sizeof(double) * (size_t)L * (size_t)Q);
    const size_t o_H = A.reserve(wide ? sizeof(double) * (size_t)ld * (size_t)Q : 0);
    const size_t o_Hd = A.reserve(wide ? sizeof(double) * (size_t)Q : 0);
    const size_t o_q = A.reserve(wide ? sizeof(double) * (size_t)Q : 0);
    SGD_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&A.base), A.used));

    SGD_HIP_TRY(hipStreamCreateWithFlags(&sx.st, hipStreamNonBlocking));
    SGD_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&sx.rec_host), sizeof(double) * kRecLen, hipHostMallocDefault));
    if (timed)
      for (hipEvent_t& e : sx.e) SGD_HIP_TRY(hipEventCreate(&e));
    st = sx.st;
    rec = sx.rec_host;
    d_x = A.at<double>(o_x);
    d_y = A.at<double>(o_y);
    d_mu = A.at<double>(o_mu);
    d_m = A.at<double>(o_m);
    d_scale = A.at<double>(o_scale);
    d_part = A.at<double>(o_part);
    d_M = A.at<double>(o_M);
    d_partial = A.at<double>(o_partial);
    d_rec = A.at<double>(o_rec);
    d_a = A.at<double>(o_a);
    d_cur = A.at<double>(o_u0);
    d_cand = A.at<double>(o_u1);
    d_U = A.at<double>(o_U);
    d_H = A.at<double>(o_H);
    d_Hd = A.at<double>(o_Hd);
    d_q = A.at<double>(o_q);
    SGD_HIP_TRY(hipMemcpyAsync(d_x, pb.x_dense, sizeof(double) * (size_t)(n * (int64_t)p), hipMemcpyHostToDevice, st));
    SGD_HIP_TRY(hipMemcpyAsync(d_y, pb.y, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
    SGD_HIP_TRY(hipMemcpyAsync(d_scale, pb.scale, sizeof(double) * (size_t)p, hipMemcpyHostToDevice, st));
    SGD_HIP_TRY(hipMemcpyAsync(d_cur, u_cur, sizeof(double) * (size_t)Q, hipMemcpyHostToDevice, st));
    SGD_HIP_TRY(hipMemcpyAsync(d_cand, u_cand, sizeof(double) * (size_t)Q, hipMemcpyHostToDevice, st));
    SGD_HIP_TRY(hipMemsetAsync(d_rec, 0, sizeof(double) * kRecLen, st));
    hipLaunchKernelGGL(cov_sum_kernel<false>, dim3((unsigned)P), dim3(kBlock), 0, st, d_x, (const int32_t*)nullptr, d_y, n, p, 1,
                       pb.centre ? 1 : 0, d_m);
    SGD_HIP_TRY(hipGetLastError());
    return SGDNET_OK;
  }

  // publish / blend: d_cand <- d_cur + t (d_cand - d_cur), its state-pass form d_a and its record
  int publish(double t) {
    if (wide) hipLaunchKernelGGL(mnewton_wide_blend_kernel, dim3(1), dim3(64), 0, st, d_cur, d_scale, p, Q, t, d_cand, d_a, d_rec);
    else hipLaunchKernelGGL(mnewton_blend_kernel, dim3(1), dim3(64), 0, st, d_cur, d_scale, p, Q, t, d_cand, d_a, d_rec);
    SGD_HIP_TRY(hipGetLastError());
    return SGDNET_OK;
  }

  // the state pass at the candidate (d_a) and its record, read back into rec
  int state_pass() {
    if (timed) SGD_HIP_TRY(hipEventRecord(sx.e[2], st));
    hipLaunchKernelGGL(mnewton_state_kernel, dim3((unsigned)state_blocks), dim3(kBlock), 0, st, d_x, d_y, d_m, d_a, n, p, K, d_mu, d_partial);
    hipLaunchKernelGGL(mnewton_finish_kernel, dim3(1), dim3(kBlock), 0, st, d_partial, state_blocks, n, d_rec);
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

  // the moments pass: d_M from d_mu of the last state pass (timed: between the events 0 and 1)
  int moments() {
    if (timed) SGD_HIP_TRY(hipEventRecord(sx.e[0], st));
    hipLaunchKernelGGL(mnewton_pair_tile_kernel, dim3((unsigned)pairs, (unsigned)chunks, (unsigned)class_pairs), dim3(kBlock), 0, st, d_x,
                       d_y, d_mu, d_m, n, p, K, rows_per_chunk, d_part);
    hipLaunchKernelGGL(mnewton_pair_reduce_kernel, dim3((unsigned)pairs, (unsigned)class_pairs), dim3(kBlock), 0, st, d_part, (int)chunks,
                       nc, d_M);
    SGD_HIP_TRY(hipGetLastError());
    if (timed) SGD_HIP_TRY(hipEventRecord(sx.e[1], st));
    return SGDNET_OK;
  }

  // wide: H, diag H and q from d_M (timed: up to the event 4)
  int wide_scale() {
    hipLaunchKernelGGL(mnewton_wide_scale_kernel, dim3((unsigned)Q), dim3(kBlock), 0, st, d_M, d_scale, p, K, ld, (double)n, d_H, d_Hd, d_q);
    SGD_HIP_TRY(hipGetLastError());
    if (timed) SGD_HIP_TRY(hipEventRecord(sx.e[4], st));
    return SGDNET_OK;
  }

  // wide: the list solve on d_H, d_Hd and d_q about d_cur
  int wide_solve(double al, double be, bool ridge, bool fit_intercept, unsigned max_sweeps, double tol) {
    const auto kernel = width == kWideNarrow ? mnewton_wide_cd_kernel<kWideNarrow> : mnewton_wide_cd_kernel<kWideFull>;
    hipLaunchKernelGGL(kernel, dim3(1), dim3((unsigned)width), 0, st, d_H, d_Hd, d_q, d_scale, p, K, ld, d_cur, al, be, ridge ? 1 : 0,
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
    if (width == 256)
      hipLaunchKernelGGL(mnewton_cd_kernel<256>, dim3(1), dim3(256), 0, st, d_M, d_scale, p, K, (double)n, d_cur, al, be, ridge ? 1 : 0,
                         fit_intercept ? 1 : 0, max_sweeps, tol, d_cand, d_a, d_rec);
    else
      hipLaunchKernelGGL(mnewton_cd_kernel<64>, dim3(1), dim3(64), 0, st, d_M, d_scale, p, K, (double)n, d_cur, al, be, ridge ? 1 : 0,
                         fit_intercept ? 1 : 0, max_sweeps, tol, d_cand, d_a, d_rec);
    SGD_HIP_TRY(hipGetLastError());
    return SGDNET_OK;
  }
};

}  // namespace

namespace {

// mnewton_run and wmnewton_run: one outer loop, one state machine (newton.hip: newton_loop).  wide: MNewtonDevice scales the
// pair moments into H in global memory and runs mnewton_wide_cd_kernel<width>; the row chunks follow wmnewton_row_chunks;
// the blend has no array of kMNewtonMaxCoordinates.  Not wide: exactly the launches multinomial Newton mode has always made.
int mnewton_loop(const MNewtonProblem& pb, bool timed, MNewtonResult* out, bool wide, int width) {
  const int p = (int)pb.p, P = p + 1, K = pb.K, L = pb.n_lambda;
  if (pb.n <= 0 || pb.p <= 0 || K < 2 || pb.p > (wide ? wmnewton_max_features(K) : mnewton_max_features(K)) || L <= 0 ||
      (wide && width != kWideNarrow && width != kWideFull) || !pb.x_dense || !pb.y || !pb.scale || !pb.b0 || !pb.alpha || !pb.beta ||
      pb.max_iter == 0) {
    set_error("%s: invalid problem", wide ? "wmnewton_run" : "mnewton_run");
    return SGDNET_EINVAL;
  }
  const int Q = K * P;
  std::vector<double> start((size_t)Q, 0.0);
  for (int k = 0; k < K; ++k) start[(size_t)k * (size_t)P + (size_t)p] = pb.b0[k];
  MNewtonDevice D;
  D.wide = wide;
  int rc = D.setup(pb, start.data(), start.data(), timed, width);
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
    SGD_HIP_TRY(hipMemcpyAsync(D.d_U + (size_t)l * (size_t)Q, D.d_cur, sizeof(double) * (size_t)Q, hipMemcpyDeviceToDevice, st));
    out->loss[(size_t)l] = loss;
    out->steps[(size_t)l] = (int32_t)steps;
    out->unconverged[(size_t)l] = converged ? 0 : 1;
  }
  out->passes = D.passes;
  out->state_ms = D.state_ms;

  out->mean.resize((size_t)p);
  out->u.resize((size_t)L * (size_t)Q);
  SGD_HIP_TRY(hipMemcpyAsync(out->mean.data(), D.d_m, sizeof(double) * (size_t)p, hipMemcpyDeviceToHost, st));
  SGD_HIP_TRY(hipMemcpyAsync(out->u.data(), D.d_U, sizeof(double) * (size_t)L * (size_t)Q, hipMemcpyDeviceToHost, st));
  SGD_HIP_TRY(hipStreamSynchronize(st));
  return SGDNET_OK;
}

}  // namespace

int mnewton_run(const MNewtonProblem& pb, bool timed, MNewtonResult* out, int width) { return mnewton_loop(pb, timed, out, false, width); }

int wmnewton_run(const MNewtonProblem& pb, bool timed, MNewtonResult* out, int width) {
  const int64_t Q = (int64_t)pb.K * (pb.p + 1);
  return mnewton_loop(pb, timed, out, true, width != 0 ? width : wmnewton_cd_width((int)std::min<int64_t>(Q, kWmnewtonMaxCoordinates)));
}

namespace {

// the geometry of a call's jobs: a function of (p, K, the groups, the number of mixes) alone
struct MCvGeometry {
  int pairs = 0, class_pairs = 0, max_chunks = 0, max_state_blocks = 0;
  std::vector<CvJob> jobs;
  std::vector<int64_t> mu_at;          // jobs + 1: where a job's mu starts, in doubles
  MCvGeometry(int64_t p, int K, const int64_t* n_t, int n_sets, int n_mix) {
    const int nc = (int)p + 2, T = (nc + kTileCols - 1) / kTileCols;
    pairs = T * (T + 1) / 2;
    class_pairs = K * (K + 1) / 2;
    jobs.resize((size_t)n_sets * (size_t)n_mix);
    mu_at.assign(jobs.size() + 1, 0);
    for (int a = 0; a < n_mix; ++a)
      for (int t = 0; t < n_sets; ++t) {
        const size_t job = (size_t)a * (size_t)n_sets + (size_t)t;
        CvJob& J = jobs[job];
        J = CvJob{};
        J.n_t = n_t[t];
        J.set = t;
        J.rows_per_chunk = dense_rows_per_chunk(J.n_t, pairs * class_pairs);
        J.chunks = (int32_t)((J.n_t + J.rows_per_chunk - 1) / J.rows_per_chunk);
        J.state_blocks = (int32_t)std::min<int64_t>(kStateMaxBlocks, (J.n_t + kBlock - 1) / kBlock);
        max_chunks = std::max(max_chunks, (int)J.chunks);
        max_state_blocks = std::max(max_state_blocks, (int)J.state_blocks);
        mu_at[job + 1] = mu_at[job] + J.n_t * K;
      }
  }
};

static_assert(kStateMaxBlocks == kMNewtonCvStateMaxBlocks && kRecLen == kMNewtonCvRecordDoubles && kTileRows == 64 && kBlock == 256,
              "mnewton.hpp: mnewton_cv_workspace_bytes counts these");

}  // namespace

// The lock-step loop: newton_cv_run's (newton.hip) around the kernels of the multinomial step.  A round: the commands go up
// in one copy, every kernel is launched once over all jobs (a job whose command does not need a kernel leaves it at once),
// the records come back in one copy, and every job's state machine moves as mnewton_run moves its one
// (newton_cv_device.hpp: cv_job_advance).  The loop ends when every job has finished its last lambda; one last launch
// stores the iterates still owed.
int mnewton_cv_run(const MNewtonCvProblem& pb, bool timed, MNewtonCvResult* out) {
  const int p = (int)pb.p, P = p + 1, nc = p + 2, K = pb.K, L = pb.n_lambda, G = pb.n_sets;
  const int64_t n = pb.n;
  if (n <= 0 || pb.p <= 0 || K < 2 || pb.p > mnewton_max_features(K) || L <= 0 || G <= 0 || pb.n_mix <= 0 || !pb.x_dense || !pb.y || !pb.start ||
      !pb.mean || !pb.scale || !pb.b0 || !pb.l2 || !pb.l1 || !pb.ridge || pb.max_iter == 0 || (int64_t)G * pb.n_mix > kNewtonCvMaxJobs ||
      (int64_t)G * pb.n_mix * (K * (K + 1) / 2) > kMNewtonCvMaxGridZ) {
    set_error("mnewton_cv_run: invalid problem");
    return SGDNET_EINVAL;
  }
  const int Q = K * P;
  std::vector<int64_t> n_t((size_t)G);
  for (int t = 0; t < G; ++t) {
    const int64_t own = pb.start[t + 1] - pb.start[t];
    n_t[(size_t)t] = pb.train_on_rest ? n - own : own;
    if (own <= 0 || n_t[(size_t)t] <= 0) {
      set_error("mnewton_cv_run: empty training set %d", t);
      return SGDNET_EINVAL;
    }
  }
  MCvGeometry geo(p, K, n_t.data(), G, pb.n_mix);
  const int jobs = (int)geo.jobs.size(), class_pairs = geo.class_pairs;
  for (CvJob& J : geo.jobs) {
    cv_job_rows(J, pb.start, n, pb.train_on_rest);
    if (J.chunks != mnewton_cv_chunks(J.n_t, (int64_t)geo.pairs * class_pairs)) {    // (what the caller sized the workspace with)
      set_error("mnewton_cv_run: the row chunks of %lld rows differ from mnewton_cv_chunks", (long long)J.n_t);
      return SGDNET_EINVAL;
    }
  }
  const int width = mnewton_cd_width(Q);

  SGD_HIP_TRY(hipSetDevice(pb.device));
  Arena A;
  const size_t o_x = A.reserve(sizeof(double) * (size_t)(n * (int64_t)p));
  const size_t o_y = A.reserve(sizeof(double) * (size_t)n);
  const size_t o_m = A.reserve(sizeof(double) * (size_t)G * (size_t)p);
  const size_t o_scale = A.reserve(sizeof(double) * (size_t)G * (size_t)p);
  const size_t o_jobs = A.reserve(sizeof(CvJob) * (size_t)jobs);
  const size_t o_cmd = A.reserve(sizeof(CvCmd) * (size_t)jobs);
  const size_t o_mu_at = A.reserve(sizeof(int64_t) * (size_t)jobs);
  const size_t o_mu = A.reserve(sizeof(double) * (size_t)geo.mu_at[(size_t)jobs]);
  const size_t o_part = A.reserve(sizeof(double) * (size_t)jobs * (size_t)class_pairs * (size_t)geo.max_chunks * (size_t)geo.pairs * kBlock);
  const size_t o_M = A.reserve(sizeof(double) * (size_t)jobs * (size_t)class_pairs * (size_t)nc * (size_t)nc);
  const size_t o_partial = A.reserve(sizeof(double) * (size_t)jobs * kStateMaxBlocks);
  const size_t o_rec = A.reserve(sizeof(double) * kRecLen * (size_t)jobs);
  const size_t o_u = A.reserve(sizeof(double) * 2 * (size_t)Q * (size_t)jobs);
  const size_t o_a = A.reserve(sizeof(double) * (size_t)Q * (size_t)jobs);
  const size_t o_U = A.reserve(sizeof(double) * (size_t)jobs * (size_t)L * (size_t)Q);
  SGD_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&A.base), A.used));
  double *d_x = A.at<double>(o_x), *d_y = A.at<double>(o_y), *d_m = A.at<double>(o_m), *d_scale = A.at<double>(o_scale),
         *d_mu = A.at<double>(o_mu), *d_part = A.at<double>(o_part), *d_M = A.at<double>(o_M), *d_partial = A.at<double>(o_partial),
         *d_rec = A.at<double>(o_rec), *d_u = A.at<double>(o_u), *d_a = A.at<double>(o_a), *d_U = A.at<double>(o_U);
  CvJob* d_jobs = A.at<CvJob>(o_jobs);
  CvCmd* d_cmd = A.at<CvCmd>(o_cmd);
  int64_t* d_mu_at = A.at<int64_t>(o_mu_at);

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
  std::vector<double> start((size_t)jobs * 2 * (size_t)Q, 0.0);
  for (int job = 0; job < jobs; ++job)
    for (int b = 0; b < 2; ++b)
      for (int k = 0; k < K; ++k)
        start[((size_t)job * 2 + (size_t)b) * (size_t)Q + (size_t)k * (size_t)P + (size_t)p] = pb.b0[(size_t)geo.jobs[(size_t)job].set * (size_t)K + (size_t)k];
  SGD_HIP_TRY(hipMemcpyAsync(d_x, pb.x_dense, sizeof(double) * (size_t)(n * (int64_t)p), hipMemcpyHostToDevice, st));
  SGD_HIP_TRY(hipMemcpyAsync(d_y, pb.y, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
  SGD_HIP_TRY(hipMemcpyAsync(d_m, pb.mean, sizeof(double) * (size_t)G * (size_t)p, hipMemcpyHostToDevice, st));
  SGD_HIP_TRY(hipMemcpyAsync(d_scale, pb.scale, sizeof(double) * (size_t)G * (size_t)p, hipMemcpyHostToDevice, st));
  SGD_HIP_TRY(hipMemcpyAsync(d_jobs, geo.jobs.data(), sizeof(CvJob) * (size_t)jobs, hipMemcpyHostToDevice, st));
  SGD_HIP_TRY(hipMemcpyAsync(d_mu_at, geo.mu_at.data(), sizeof(int64_t) * (size_t)jobs, hipMemcpyHostToDevice, st));
  SGD_HIP_TRY(hipMemcpyAsync(d_u, start.data(), sizeof(double) * start.size(), hipMemcpyHostToDevice, st));
  SGD_HIP_TRY(hipMemsetAsync(d_rec, 0, sizeof(double) * kRecLen * (size_t)jobs, st));

  out->loss.assign((size_t)jobs * (size_t)L, 0.0);
  out->unconverged.assign((size_t)jobs * (size_t)L, 0);
  out->passes.assign((size_t)jobs, 0.0);
  out->steps.assign((size_t)jobs, 0.0);
  out->halvings.assign((size_t)jobs, 0.0);
  out->sweeps = 0.0;
  out->rounds = 0;
  out->moments_ms = out->cd_ms = out->state_ms = 0.f;

  std::vector<CvJobState> state((size_t)jobs);
  const int fit_intercept = pb.fit_intercept ? 1 : 0;
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
      hipLaunchKernelGGL(mnewton_cv_pair_tile_kernel, dim3((unsigned)geo.pairs, (unsigned)geo.max_chunks, (unsigned)(jobs * class_pairs)),
                         dim3(kBlock), 0, st, d_cmd, d_jobs, d_mu_at, d_x, d_y, d_mu, d_m, n, p, K, geo.max_chunks, d_part);
      hipLaunchKernelGGL(mnewton_cv_pair_reduce_kernel, dim3((unsigned)geo.pairs, (unsigned)(jobs * class_pairs)), dim3(kBlock), 0, st, d_cmd,
                         d_jobs, d_part, class_pairs, geo.max_chunks, nc, d_M);
    }
    if (timed) SGD_HIP_TRY(hipEventRecord(sx.e[1], st));
    // (the inner solve's kernel also stores the iterates owed to U: it runs in every round)
    if (width == 256)
      hipLaunchKernelGGL(mnewton_cv_cd_kernel<256>, dim3((unsigned)jobs), dim3(256), 0, st, d_cmd, d_jobs, d_M, d_scale, p, K, L, fit_intercept,
                         kNewtonMaxSweeps, pb.tol, d_u, d_a, d_rec, d_U);
    else
      hipLaunchKernelGGL(mnewton_cv_cd_kernel<64>, dim3((unsigned)jobs), dim3(64), 0, st, d_cmd, d_jobs, d_M, d_scale, p, K, L, fit_intercept,
                         kNewtonMaxSweeps, pb.tol, d_u, d_a, d_rec, d_U);
    if (any_blend)
      hipLaunchKernelGGL(mnewton_cv_blend_kernel, dim3((unsigned)jobs), dim3(64), 0, st, d_cmd, d_jobs, d_scale, p, Q, d_u, d_a, d_rec);
    if (timed) SGD_HIP_TRY(hipEventRecord(sx.e[2], st));
    if (live > 0) {
      hipLaunchKernelGGL(mnewton_cv_state_kernel, dim3((unsigned)geo.max_state_blocks, (unsigned)jobs), dim3(kBlock), 0, st, d_cmd, d_jobs,
                         d_mu_at, d_x, d_y, d_m, d_a, n, p, K, d_mu, d_partial);
      hipLaunchKernelGGL(mnewton_cv_finish_kernel, dim3((unsigned)jobs), dim3(kBlock), 0, st, d_cmd, d_jobs, d_partial, d_rec);
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
      SGD_HIP_TRY(hipEventElapsedTime(&ms, sx.e[1], sx.e[2]));
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
  out->u.resize((size_t)jobs * (size_t)L * (size_t)Q);
  SGD_HIP_TRY(hipMemcpyAsync(out->u.data(), d_U, sizeof(double) * out->u.size(), hipMemcpyDeviceToHost, st));
  SGD_HIP_TRY(hipStreamSynchronize(st));
  return SGDNET_OK;
}

// Diagnostics (include/sgdnet_hip.h): one outer step through the steps above, every output copied back.  The state is
// taken at the candidate io->u; the moments are those of that state; the inner solve runs on them about io->u_cur.
// wide (sgdnet_wmnewton_probe): the steps of a wide fit, and what the scale kernel wrote is copied between it and the solve.
namespace {

template <class IO>
int mnewton_probe_steps(const MNewtonProblem& pb, IO* io, bool wide, int width, double* H_out, double* Hd_out, double* q_out) {
  MNewtonDevice D;
  D.wide = wide;
  int rc = D.setup(pb, io->u_cur, io->u, false, width);
  if (rc) return rc;
  hipStream_t st = D.st;
  const size_t Q = (size_t)D.Q;
  double rec[kRecLen];
  // a candidate as it was published: itself, its state-pass form and fields of the record
  auto fetch = [&](double* u_out, double* a_out, double* rec_out, int rec_from, int rec_len) -> int {
    if (u_out) SGD_HIP_TRY(hipMemcpyAsync(u_out, D.d_cand, sizeof(double) * Q, hipMemcpyDeviceToHost, st));
    if (a_out) SGD_HIP_TRY(hipMemcpyAsync(a_out, D.d_a, sizeof(double) * Q, hipMemcpyDeviceToHost, st));
    SGD_HIP_TRY(hipMemcpyAsync(rec, D.d_rec, sizeof(double) * kRecLen, hipMemcpyDeviceToHost, st));
    SGD_HIP_TRY(hipStreamSynchronize(st));
    std::copy(rec + rec_from, rec + rec_from + rec_len, rec_out);
    return SGDNET_OK;
  };
  if ((rc = D.publish(1.0)) || (rc = fetch(io->pub_u, io->pub_a, io->pub_rec, kRecHalfSq, 4))) return rc;
  if (io->mean) SGD_HIP_TRY(hipMemcpyAsync(io->mean, D.d_m, sizeof(double) * (size_t)D.p, hipMemcpyDeviceToHost, st));
  if ((rc = D.state_pass())) return rc;
  io->loss = D.rec[kRecLoss];
  if (io->mu) SGD_HIP_TRY(hipMemcpyAsync(io->mu, D.d_mu, sizeof(double) * (size_t)D.n * (size_t)D.K, hipMemcpyDeviceToHost, st));
  if ((rc = D.moments())) return rc;
  if (io->M)
    SGD_HIP_TRY(hipMemcpyAsync(io->M, D.d_M, sizeof(double) * (size_t)D.class_pairs * (size_t)D.nc * (size_t)D.nc, hipMemcpyDeviceToHost, st));
  const double be = io->ridge ? 0.0 : io->l1;
  if (wide) {
    if ((rc = D.wide_scale())) return rc;
    if (H_out) SGD_HIP_TRY(hipMemcpyAsync(H_out, D.d_H, sizeof(double) * (size_t)D.ld * Q, hipMemcpyDeviceToHost, st));
    if (Hd_out) SGD_HIP_TRY(hipMemcpyAsync(Hd_out, D.d_Hd, sizeof(double) * Q, hipMemcpyDeviceToHost, st));
    if (q_out) SGD_HIP_TRY(hipMemcpyAsync(q_out, D.d_q, sizeof(double) * Q, hipMemcpyDeviceToHost, st));
    rc = D.wide_solve(io->l2, be, io->ridge != 0, io->fit_intercept != 0, io->max_sweeps, io->tol);
  } else {
    rc = D.inner_solve(io->l2, be, io->ridge != 0, io->fit_intercept != 0, io->max_sweeps, io->tol);
  }
  if (rc || (rc = fetch(io->cd_u, io->cd_a, io->cd_rec, 0, kRecLen))) return rc;
  // the candidate again, blended with the iterate at the caller's t
  SGD_HIP_TRY(hipMemcpyAsync(D.d_cand, io->u, sizeof(double) * Q, hipMemcpyHostToDevice, st));
  if ((rc = D.publish(io->t)) || (rc = fetch(io->blend_u, io->blend_a, io->blend_rec, kRecHalfSq, 4))) return rc;
  return SGDNET_OK;
}

}  // namespace

int mnewton_probe(const MNewtonProblem& pb, sgdnet_mnewton_probe_io* io) {
  return mnewton_probe_steps(pb, io, false, io->width, nullptr, nullptr, nullptr);
}

int wmnewton_probe(const MNewtonProblem& pb, sgdnet_wmnewton_probe_io* io) {
  const int64_t Q = (int64_t)pb.K * (pb.p + 1);
  const int width = io->width != 0 ? io->width : wmnewton_cd_width((int)std::min<int64_t>(Q, kWmnewtonMaxCoordinates));
  io->ld = (int)wide_leading_dim(Q);
  return mnewton_probe_steps(pb, io, true, width, io->H, io->Hd, io->q);
}

}  // namespace sgdnet

extern "C" int sgdnet_mnewton_max_features(int n_classes) { return sgdnet::mnewton_max_features(n_classes); }
extern "C" int sgdnet_wmnewton_max_features(int n_classes) { return sgdnet::wmnewton_max_features(n_classes); }
