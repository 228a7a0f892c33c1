// Covariance mode (SGDNET_MODE_COVARIANCE): the Gaussian elastic-net path of one response from X'X and X'y.
//
// Once the centred cross-products are known the whole lambda path is a p x p problem; the samples are read once.
//
//   moments    C_jk = sum_i (x_ij - m_j)(x_ik - m_k),  c_j = sum_i (x_ij - m_j) y~_i      (f64, upper triangle)
//              m_j the column mean (cov_sum_kernel, a first reduction) or 0 (no intercept and no standardisation);
//              y~ the response as the driver preprocessed it.  Deviations are formed BEFORE they are multiplied:
//              raw X'X - n m m' cancels when |mean| >> sd.
//              dense x   cov_dense_tile_kernel: a workgroup owns a pair of 16-column tiles (y~ is column p) and a
//                        chunk of rows, stages 64 rows of both tiles in LDS (reads coalesced along the columns of the
//                        column-major matrix) and thread (a, b) accumulates deviation a x deviation b in row order;
//                        cov_reduce_kernel adds the chunks' partial tiles in chunk order.  A plain multiply-add tile,
//                        not the f64 MFMA: profiles/covariance_abalone.txt has its time.
//              sparse x  cov_sparse_pair_kernel: a workgroup owns a pair of columns (j, k), centred implicitly:
//                          C_jk = sum_{J and K} d_ij d_ik - m_k sum_{J \ K} d_ij - m_j sum_{K \ J} d_ik
//                                 + (n - |J or K|) m_j m_k,        d = stored value - mean,
//                        every sum a sum of deviations over stored entries (membership by binary search in the other
//                        column's ascending row indices); c_j = sum_J d_ij y~_i - m_j sum_{not J} y~_i.
//   path       cov_path_kernel: ONE wavefront keeps S = C / (n sd sd') (packed triangle), c~ = c / (n sd), w and the
//              running gradient g = S w - c~ in LDS for the whole path (covariance.hpp: the budget behind
//              sgdnet_covariance_max_features) and runs cyclic coordinate descent, warm-started lambda to lambda:
//                w_j <- prox(S_jj w_j - g_j) / (S_jj + alpha),   g <- g + S[:, j] (w_j_new - w_j_old)
//              in the driver's units (sgdnet_amd/kkt.py): alpha = (1 - mix) lambda / sd(y), the soft threshold
//              beta = mix lambda / sd(y), none for the ridge functor.  A sweep ends with the reference's
//              ConvergenceCheck (max|dw| / max|w| <= tol; all zero counts as converged: solver.cpp read_convergence).
//
//   folds      covariance_cv_run: every (training set, mix) path of a cross-validation in one launch.  Rows carry a
//              group id; the same kernels leave one moment matrix per group of the augmented rows [x - a | y - a_y | 1]
//              about ONE centre a (the whole-data means), so that the last column holds the group's sums of deviations
//              and its corner n_g.  dense x: the rows are sorted by group (a stable counting sort on the host) and no
//              row chunk straddles a group; sparse x: the pair kernel's third grid dimension is the group and stored
//              entries of other groups' rows are skipped.  cov_assemble_kernel pools the groups of a training set T
//              (one group, or the total -- summed in group order -- minus one) and re-centres to T's own means t,
//              d = t - a:   M^T_jk = C^T_jk - d_j s^T_k - d_k s^T_j + n_T d_j d_k   (s^T / n_T is of the
//              order of the columns' sd, not of their mean, so nothing cancels), then writes what cov_path_kernel reads;
//              the path kernel takes its job (mix, T) from blockIdx.x: one wavefront, one CU's LDS, per job.
//
//   responses  mcovariance_run (SGDNET_MODE_MCOVARIANCE): K responses of an mgaussian fit share S.  The moment kernels take a
//              response count (columns p .. p + K - 1 of the augmented matrix; one response is the case above, bit for
//              bit) and cov_group_path_kernel runs cyclic BLOCK coordinate descent, a block the K coefficients of a
//              feature: the group lasso with its l2 part, closed form per block (covariance.hpp has the LDS budget).
//              mcovariance_cv_run: the folds of an mgaussian cross-validation the same way.  The augmented rows are
//              [x - a | y_1 - a_y1 .. y_K - a_yK | 1], a group's matrix is (p + K + 1)^2 (sparse x: its K x K response block, the K
//              sums and n_g from cov_group_responses_kernel), mcov_assemble_kernel re-centres all p + K columns to T's own
//              means -- the responses always: the null model's intercepts -- and scales a response only with
//              standardize_response, and cov_group_path_kernel takes its job (mix, T) from blockIdx.x.
//
//   wide       wcovariance_run (SGDNET_MODE_WCOVARIANCE): beyond 198 features S does not fit one workgroup's LDS.
//              wide_scale_kernel writes it to global memory as a full symmetric matrix and cov_wide_path_kernel keeps
//              only vectors and a list of the coordinates that can move in LDS (covariance.hpp has the budget): a
//              moving coordinate reads its column of S, nothing else is touched.  The list compaction, the column move
//              and the scale kernel are wide_cd_device.hpp's, shared with newton.hip; the geometry is wide_layout.hpp's.
//              wmcovariance_run (SGDNET_MODE_WMCOVARIANCE) is the same step for the K responses: cov_wide_group_path_kernel
//              runs cov_group_path_kernel's block descent over the list, one 16-byte read of a column serving all K.
//              wcovariance_cv_run: the folds of the wide mode.  The group moments pass above (p + 2 columns, the wide row
//              chunks cut at the groups' ends); wcov_cv_stats_kernel (per T: s, d, scales, means, penalties) and
//              wcov_cv_assemble_kernel (per column and T) do cov_assemble_kernel's pooling and re-centring straight into
//              every training set's S_T, diag S_T and c~_T in global memory; cov_wide_cv_path_kernel, a second entry around
//              cov_wide_path_kernel's body, takes its job (mix, T) from blockIdx.x: one workgroup, one CU, per job.
//              wmcovariance_cv_run: the same for the K responses.  The group moments of mcovariance_cv_run (p + K + 1
//              columns, the wide row chunks), wmcov_cv_stats_kernel and wmcov_cv_assemble_kernel for mcov_assemble_kernel's
//              pooling, and cov_wide_group_cv_path_kernel, a second entry around cov_wide_group_path_kernel's body.
//
// No floating-point atomic anywhere and every reduction in an order fixed by (n, p, K, nnz, fold): the same input gives the
// same bits (the contract of gradient.hip).
#include <algorithm>
#include <numeric>
#include <vector>

#include "common.hpp"
#include "covariance.hpp"
#include "moments_device.hpp"
#include "wide_cd_device.hpp"

namespace sgdnet {
namespace {

// blockIdx.x: the pair (tj <= tk) of column tiles of the augmented matrix, blockIdx.y: the chunk of rows.
// One fit: ncols = p + nresp, the matrix is [x - mu | y_1 .. y_nresp] (y as the driver preprocessed it, n x nresp column-major),
// chunk c is rows [c rows_per_chunk, ...).
// Group moments: ncols = p + nresp + 1, [x - mu | y_r - mean(y_r) | 1] (the mean of response r at mu[p + nresp + r]), chunk c is the
// sorted rows perm[chunk_begin[c] .. chunk_begin[c + 1]).
__global__ __launch_bounds__(kBlock) void cov_dense_tile_kernel(const double* __restrict__ x, const double* __restrict__ y,
                                                                 const double* __restrict__ mu, int64_t n, int p, int nresp,
                                                                 int ncols, int64_t rows_per_chunk, const int64_t* __restrict__ perm,
                                                                 const int64_t* __restrict__ chunk_begin, double* __restrict__ part) {
  __shared__ double A[kTileCols][kTileRows + 1], B[kTileCols][kTileRows + 1];
  const int tid = threadIdx.x;
  const int T = (ncols + kTileCols - 1) / kTileCols;
  int pair = blockIdx.x, tj = 0;
  while (pair >= T - tj) {
    pair -= T - tj;
    ++tj;
  }
  const int tk = tj + pair;
  const int ta = tid & (kTileCols - 1), tb = tid / kTileCols;
  int64_t r0, r1;
  if (chunk_begin) {
    r0 = chunk_begin[blockIdx.y];
    r1 = chunk_begin[blockIdx.y + 1];
  } else {
    r0 = (int64_t)blockIdx.y * rows_per_chunk;
    r1 = r0 + rows_per_chunk < n ? r0 + rows_per_chunk : n;
  }
  const bool grouped = perm != nullptr;
  auto dev = [&](int a, int64_t i) -> double {
    if (i >= r1 || a >= ncols) return 0.0;
    if (a >= p + nresp) return 1.0;
    const int64_t r = grouped ? perm[i] : i;
    if (a < p) return x[r + (int64_t)a * n] - mu[a];
    const double yr = y[r + (int64_t)(a - p) * n];
    return grouped ? yr - mu[a + nresp] : yr;
  };
  double acc = 0.0;
  for (int64_t base = r0; base < r1; base += kTileRows) {
    for (int e = tid; e < kTileCols * kTileRows; e += kBlock) {
      const int row = e & (kTileRows - 1), col = e / kTileRows;
      A[col][row] = dev(tj * kTileCols + col, base + row);
      B[col][row] = dev(tk * kTileCols + col, base + row);
    }
    __syncthreads();
    for (int i = 0; i < kTileRows; ++i) acc += A[ta][i] * B[tb][i];
    __syncthreads();
  }
  part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kBlock + tid] = acc;
}

// Group moments of the response (sparse x; the dense tile kernel has them as columns p and p + 1): blockIdx.x = group g,
// M[g] gets sum (y - a_y)^2 at (p, p), sum (y - a_y) at (p, p + 1) and n_g at (p + 1, p + 1), each over the rows of g in row order
__global__ __launch_bounds__(kBlock) void cov_group_response_kernel(const double* __restrict__ y, const int32_t* __restrict__ fold,
                                                                     const double* __restrict__ mu, int64_t n, int p,
                                                                     double* __restrict__ M) {
  __shared__ double sh[kBlock];
  const int g = blockIdx.x, Pa = p + 2;
  const double ay = mu[p + 1];
  double s = 0.0, q = 0.0, c = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += kBlock)
    if (fold[i] == g) {
      const double d = y[i] - ay;
      s += d;
      q += d * d;
      c += 1.0;
    }
  s = block_sum(s, sh);
  q = block_sum(q, sh);
  c = block_sum(c, sh);
  if (threadIdx.x == 0) {
    double* Mg = M + (size_t)g * Pa * Pa;
    Mg[(size_t)p * Pa + p] = q;
    Mg[(size_t)p * Pa + p + 1] = s;
    Mg[(size_t)(p + 1) * Pa + p] = s;
    Mg[(size_t)(p + 1) * Pa + p + 1] = c;
  }
}

// mu[p + K + r] = the mean of response r from its sum mu[p + r] (cov_sum_kernel leaves it itself for one response)
__global__ void cov_response_centre_kernel(double* __restrict__ mu, int64_t n, int p, int K) {
  for (int r = threadIdx.x; r < K; r += blockDim.x) mu[p + K + r] = mu[p + r] / (double)n;
}

// cov_group_response_kernel for K responses (y is n x K, column-major; a_r = mu[p + K + r]): blockIdx.x = response r,
// blockIdx.y = response s >= r, blockIdx.z = group g.  M[g] is (p + K + 1) x (p + K + 1) and gets sum (y_r - a_r)(y_s - a_s) at
// (p + r, p + s) and (p + s, p + r); the block r = s also leaves sum (y_r - a_r) at (p + r, p + K) and (p + K, p + r), and the
// block r = s = 0 n_g in the corner: each over the rows of g in row order
__global__ __launch_bounds__(kBlock) void cov_group_responses_kernel(const double* __restrict__ y, const int32_t* __restrict__ fold,
                                                                      const double* __restrict__ mu, int64_t n, int p, int K,
                                                                      double* __restrict__ M) {
  __shared__ double sh[kBlock];
  const int r = blockIdx.x, t = blockIdx.y, g = blockIdx.z, Pa = p + K + 1, one = p + K;
  if (t < r) return;
  const double ar = mu[p + K + r], at = mu[p + K + t];
  const double* yr = y + (int64_t)r * n;
  const double* yt = y + (int64_t)t * n;
  double s = 0.0, q = 0.0, c = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += kBlock)
    if (fold[i] == g) {
      const double d = yr[i] - ar;
      s += d;
      q += d * (yt[i] - at);
      c += 1.0;
    }
  s = block_sum(s, sh);
  q = block_sum(q, sh);
  c = block_sum(c, sh);
  if (threadIdx.x == 0) {
    double* Mg = M + (size_t)g * Pa * Pa;
    Mg[(size_t)(p + r) * Pa + p + t] = q;
    Mg[(size_t)(p + t) * Pa + p + r] = q;
    if (r == t) {
      Mg[(size_t)(p + r) * Pa + one] = s;
      Mg[(size_t)one * Pa + p + r] = s;
      if (r == 0) Mg[(size_t)one * Pa + one] = c;
    }
  }
}

// blockIdx.x = column j < p, blockIdx.y = column k in [j, p + nresp); k = p + r is response r (y is n x nresp, column-major;
// mu[p + r] its sum) and M is (p + nresp) x (p + nresp), its response-by-response block left alone.
// kGrouped: blockIdx.z = group g, only the stored entries whose row is in g count, n becomes n_g, response r is
// y_r - a_r (a_r = mu[p + nresp + r]), k runs to p + nresp (the column of ones: the group's sum of deviations) and M[g] is
// (p + nresp + 1) x (p + nresp + 1) with the responses' own entries already in place (cov_group_response_kernel; several
// responses: cov_group_responses_kernel).
template <bool kGrouped>
__global__ __launch_bounds__(kBlock) void cov_sparse_pair_kernel(const int32_t* __restrict__ colptr, const int32_t* __restrict__ rowidx,
                                                                  const double* __restrict__ val, const double* __restrict__ y,
                                                                  const double* __restrict__ mu, int64_t n, int p, int nresp,
                                                                  const int32_t* __restrict__ fold, double* __restrict__ M) {
  __shared__ double sh[kBlock];
  const int one = p + nresp;            // kGrouped: the column of ones
  const int j = blockIdx.x, k = blockIdx.y, nc = kGrouped ? one + 1 : p + nresp, tid = threadIdx.x;
  const int g = kGrouped ? (int)blockIdx.z : 0;
  if (k < j) return;
  if (kGrouped) M += (size_t)g * nc * nc;
  auto mine = [&](int32_t r) -> bool { return !kGrouped || fold[r] == g; };
  const int q0 = colptr[j], q1 = colptr[j + 1];
  const double mj = mu[j];
  if (kGrouped ? (k >= p && k < one) : k >= p) {
    const double ay = kGrouped ? mu[k + nresp] : 0.0;
    const double* yk = y + (int64_t)(k - p) * n;
    double a = 0.0, ys = 0.0;
    for (int q = q0 + tid; q < q1; q += kBlock) {
      if (!mine(rowidx[q])) continue;
      const double yi = kGrouped ? yk[rowidx[q]] - ay : yk[rowidx[q]];
      a += (val[q] - mj) * yi;
      ys += yi;
    }
    a = block_sum(a, sh);
    ys = block_sum(ys, sh);
    if (tid == 0) {
      // the response over the samples NOT stored: none, or all - stored
      const double rest = kGrouped ? M[(size_t)k * nc + one] - ys : ((int64_t)(q1 - q0) == n ? 0.0 : mu[k] - ys);
      const double c = a - mj * rest;
      M[(size_t)j * nc + k] = c;
      M[(size_t)k * nc + j] = c;
    }
    return;
  }
  if (kGrouped && k == one) {            // the sum of the group's deviations: stored entries, then the implicit -mj
    double a = 0.0, cnt = 0.0;
    for (int q = q0 + tid; q < q1; q += kBlock)
      if (mine(rowidx[q])) {
        a += val[q] - mj;
        cnt += 1.0;
      }
    a = block_sum(a, sh);
    cnt = block_sum(cnt, sh);
    if (tid == 0) {
      const double c = a - (M[(size_t)one * nc + one] - cnt) * mj;
      M[(size_t)j * nc + one] = c;
      M[(size_t)one * nc + j] = c;
    }
    return;
  }
  const int s0 = colptr[k], s1 = colptr[k + 1];
  const double mk = mu[k];
  double both = 0.0, only_j = 0.0, only_k = 0.0, cnt = 0.0, cnt_j = 0.0, cnt_k = 0.0;
  for (int q = q0 + tid; q < q1; q += kBlock) {
    const int32_t r = rowidx[q];
    if (!mine(r)) continue;
    cnt_j += 1.0;
    const double d = val[q] - mj;
    const int pos = j == k ? q : lower_bound_row(rowidx, s0, s1, r);
    if (pos < s1 && rowidx[pos] == r) {
      both += d * (val[pos] - mk);
      cnt += 1.0;
    } else {
      only_j += d;
    }
  }
  if (j != k)
    for (int s = s0 + tid; s < s1; s += kBlock) {
      const int32_t r = rowidx[s];
      if (!mine(r)) continue;
      cnt_k += 1.0;
      const int pos = lower_bound_row(rowidx, q0, q1, r);
      if (!(pos < q1 && rowidx[pos] == r)) only_k += val[s] - mk;
    }
  both = block_sum(both, sh);
  only_j = block_sum(only_j, sh);
  only_k = block_sum(only_k, sh);
  cnt = block_sum(cnt, sh);
  if (kGrouped) {
    cnt_j = block_sum(cnt_j, sh);
    cnt_k = j == k ? cnt_j : block_sum(cnt_k, sh);
  }
  if (tid == 0) {
    const double in_neither = kGrouped ? M[(size_t)one * nc + one] - (cnt_j + cnt_k - cnt)
                                       : (double)n - ((double)(q1 - q0) + (double)(s1 - s0) - cnt);
    const double c = both - mk * only_j - mj * only_k + in_neither * mj * mk;
    M[(size_t)j * nc + k] = c;
    M[(size_t)k * nc + j] = c;
  }
}

// total[e] = sum_g M[g][e], in group order
__global__ __launch_bounds__(kBlock) void cov_total_kernel(const double* __restrict__ M, int n_groups, int elems, double* __restrict__ total) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= elems) return;
  double s = 0.0;
  for (int g = 0; g < n_groups; ++g) s += M[(size_t)g * elems + e];
  total[e] = s;
}

// Is a column (a feature or a response) constant on training set T?  (DESIGN.md 4.5 has the derivation.)  Its re-centred
// square q = C_jj - 2 d_j s_j + n_T d_j^2 is formed about the WHOLE-data centre: for a column that is constant on T and not on
// the data, C_jj, d_j s_j and n_T d_j^2 are each n_T (c - a)^2 and q is their rounding noise, of either sign.  "q > 0" cannot
// tell that from a variance; the bound of that noise can.  With every deviation on T the same double, C_jj and s_j are sums of
// n_T equal terms (rest: less a group, out of a total of G terms), each within gamma_(n_T + G) of its magnitude a_c, a_s
// (rest: |total| + |group|), and the expression adds three products and three sums of them:
//   |q| <= (n_T + G + 8) 2^-52 (a_c + 2 |d| a_s + n_T d^2)        (2^-52 = 2 u: the factor 2 pays for the second-order terms)
// A column at or below that is constant: scale 1, and exact zeros in what the path kernel reads, as the separate fit on x[T]
// has them.  n_summed: G with rest, 0 without.
__device__ __forceinline__ bool cov_constant_on_set(double q, double a_c, double a_s, double d, double nT, int n_summed) {
  const double tol = (nT + (double)n_summed + 8.0) * 0x1p-52 * (a_c + 2.0 * fabs(d) * a_s + nT * d * d);
  return !(q > tol);
}

// blockIdx.x = training set T: group T alone, or (rest) the total less group T.  From the (p + 2) x (p + 2) moments about the
// common centre a to what cov_path_kernel reads for x[T], y[T] as fit_covariance (driver_direct.cpp) / prepare_response (driver.cpp) would
// prepare them: the cross-products about T's own means t = a + d, the y column divided by sd_T(y), the features' sd over T,
// n_T, and the penalties of every mix in the units of the preprocessed response.
//   Mt     G x (p + 1) x (p + 1)      scale  G x p      mean  G x (p + 1): t (0 where the features are not centred), mean_T(y)
//   tstat  3 x G: n_T | sd_T(y) (0 -> 1) | y~'y~         alpha, beta  jobs x n_lambda, job = mix * G + T      ridge  jobs
__global__ __launch_bounds__(kBlock) void cov_assemble_kernel(const double* __restrict__ Mg, const double* __restrict__ total,
                                                               const double* __restrict__ mu, int n_groups, int p, int rest, int centre,
                                                               int standardize, const double* __restrict__ mix,
                                                               const double* __restrict__ lambda, int n_mix, int n_lambda,
                                                               double* __restrict__ Mt, double* __restrict__ scale, double* __restrict__ mean,
                                                               double* __restrict__ tstat, double* __restrict__ alpha,
                                                               double* __restrict__ beta, int32_t* __restrict__ ridge) {
  __shared__ double s[kCovMaxFeatures + 1], d[kCovMaxFeatures + 1];
  __shared__ int cst[kCovMaxFeatures + 1];      // the column is constant on T (cov_constant_on_set)
  const int t = blockIdx.x, tid = threadIdx.x, P1 = p + 1, Pa = p + 2;
  const double* Ct = Mg + (size_t)t * Pa * Pa;
  auto C = [&](int j, int k) -> double {
    const double v = Ct[(size_t)j * Pa + k];
    return rest ? total[(size_t)j * Pa + k] - v : v;
  };
  auto magnitude = [&](int j, int k) -> double {
    const double v = fabs(Ct[(size_t)j * Pa + k]);
    return rest ? fabs(total[(size_t)j * Pa + k]) + v : v;
  };
  const double nT = C(p + 1, p + 1);
  for (int j = tid; j < P1; j += kBlock) {
    s[j] = C(j, p + 1);
    d[j] = (j == p || centre) ? s[j] / nT : 0.0;
  }
  __syncthreads();
  auto recentred = [&](int j, int k) -> double { return C(j, k) - d[j] * s[k] - d[k] * s[j] + nT * d[j] * d[k]; };
  for (int j = tid; j < P1; j += kBlock)
    cst[j] = cov_constant_on_set(recentred(j, j), magnitude(j, j), magnitude(j, p + 1), d[j], nT, rest ? n_groups : 0) ? 1 : 0;
  __syncthreads();
  const double var_y = recentred(p, p) / nT;
  const double sd_y = cst[p] ? 1.0 : sqrt(var_y);
  for (int e = tid; e < P1 * P1; e += kBlock) {
    const int j = e / P1, k = e - j * P1;
    double m = recentred(j, k);
    if (j == p) m /= sd_y;
    if (k == p) m /= sd_y;
    Mt[(size_t)t * P1 * P1 + e] = (cst[j] || cst[k]) ? 0.0 : m;
  }
  for (int j = tid; j < p; j += kBlock) {
    const double v = recentred(j, j) / nT;
    scale[(size_t)t * p + j] = (standardize && !cst[j]) ? sqrt(v) : 1.0;
    mean[(size_t)t * P1 + j] = centre ? mu[j] + d[j] : 0.0;
  }
  if (tid == 0) {
    mean[(size_t)t * P1 + p] = mu[p + 1] + d[p];
    tstat[t] = nT;
    tstat[n_groups + t] = sd_y;
    tstat[2 * n_groups + t] = cst[p] ? 0.0 : recentred(p, p) / sd_y / sd_y;
  }
  for (int e = tid; e < n_mix * n_lambda; e += kBlock) {
    const int a = e / n_lambda, l = e - a * n_lambda;
    const size_t at = ((size_t)a * n_groups + t) * n_lambda + l;
    alpha[at] = (1.0 - mix[a]) * lambda[e] / sd_y;
    beta[at] = mix[a] * lambda[e] / sd_y;
    if (l == 0) ridge[(size_t)a * n_groups + t] = mix[a] == 0.0 ? 1 : 0;
  }
}

// cov_assemble_kernel for K responses: blockIdx.x = training set T, from the (p + K + 1) x (p + K + 1) group moments about the
// common centre to what cov_group_path_kernel reads for x[T], y[T] as fit_mcovariance (driver_direct.cpp) would prepare
// them: every response less its own mean over T (the null model's intercept), divided by its sd over T only with
// standardize_response; the fit stays on that scale, so the penalties are those of the mix and the lambda alone.
//   Mt     G x p x (p + K): rows j < p of the (p + K) x (p + K) matrix (all the path kernel reads)      scale  G x p
//   mean   G x (p + K): the means of x over T (0 where the features are not centred), then those of the responses AS THE FIT
//          SEES THEM (the null model's intercepts: mean_T(y_r), or 0 on the standardised scale)
//   tstat  3 x G: n_T | y~'y~ = sum_r y~_r'y~_r | the null deviance of y[T] as it came = sum_r |y_r - mean_T(y_r)|^2, both in
//          the order r = 0 .. K - 1           l2, l1  jobs x n_lambda, job = mix * G + T      ridge  jobs
// The staging arrays (the sums s and the shifts d of the p + K columns, then their constant-on-T flags) are 2 (p + K) doubles
// and p + K ints of dynamic LDS.
__global__ __launch_bounds__(kBlock) void mcov_assemble_kernel(const double* __restrict__ Mg, const double* __restrict__ total,
                                                                const double* __restrict__ mu, int n_groups, int p, int K, int rest,
                                                                int centre, int standardize, int standardize_response,
                                                                const double* __restrict__ mix, const double* __restrict__ lambda,
                                                                int n_mix, int n_lambda, double* __restrict__ Mt,
                                                                double* __restrict__ scale, double* __restrict__ mean,
                                                                double* __restrict__ tstat, double* __restrict__ l2,
                                                                double* __restrict__ l1, int32_t* __restrict__ ridge) {
  extern __shared__ double staged[];
  const int t = blockIdx.x, tid = threadIdx.x, nc = p + K, Pa = nc + 1;
  double* s = staged;
  double* d = staged + nc;
  int* cst = reinterpret_cast<int*>(staged + 2 * nc);      // the column is constant on T (cov_constant_on_set)
  const double* Ct = Mg + (size_t)t * Pa * Pa;
  auto C = [&](int j, int k) -> double {
    const double v = Ct[(size_t)j * Pa + k];
    return rest ? total[(size_t)j * Pa + k] - v : v;
  };
  auto magnitude = [&](int j, int k) -> double {
    const double v = fabs(Ct[(size_t)j * Pa + k]);
    return rest ? fabs(total[(size_t)j * Pa + k]) + v : v;
  };
  const double nT = C(nc, nc);
  for (int j = tid; j < nc; j += kBlock) {
    s[j] = C(j, nc);
    d[j] = (j >= p || centre) ? s[j] / nT : 0.0;
  }
  __syncthreads();
  auto recentred = [&](int j, int k) -> double { return C(j, k) - d[j] * s[k] - d[k] * s[j] + nT * d[j] * d[k]; };
  for (int j = tid; j < nc; j += kBlock)
    cst[j] = cov_constant_on_set(recentred(j, j), magnitude(j, j), magnitude(j, nc), d[j], nT, rest ? n_groups : 0) ? 1 : 0;
  __syncthreads();
  // the sd response r is divided by (1 without standardize_response; a response constant on T: 1)
  auto sd_y = [&](int r) -> double {
    if (!standardize_response || cst[p + r]) return 1.0;
    return sqrt(recentred(p + r, p + r) / nT);
  };
  for (int e = tid; e < p * nc; e += kBlock) {
    const int j = e / nc, k = e - j * nc;
    double m = recentred(j, k);
    if (k >= p) m /= sd_y(k - p);
    Mt[(size_t)t * p * nc + e] = (cst[j] || cst[k]) ? 0.0 : m;
  }
  for (int j = tid; j < p; j += kBlock) {
    const double v = recentred(j, j) / nT;
    scale[(size_t)t * p + j] = (standardize && !cst[j]) ? sqrt(v) : 1.0;
    mean[(size_t)t * nc + j] = centre ? mu[j] + d[j] : 0.0;
  }
  for (int r = tid; r < K; r += kBlock) mean[(size_t)t * nc + p + r] = standardize_response ? 0.0 : mu[nc + r] + d[p + r];
  if (tid == 0) {
    double yy = 0.0, nulldev = 0.0;
    for (int r = 0; r < K; ++r) {
      const double q = cst[p + r] ? 0.0 : recentred(p + r, p + r), sd = sd_y(r);
      nulldev += q;
      yy += q / sd / sd;
    }
    tstat[t] = nT;
    tstat[n_groups + t] = yy;
    tstat[2 * n_groups + t] = nulldev;
  }
  for (int e = tid; e < n_mix * n_lambda; e += kBlock) {
    const int a = e / n_lambda, l = e - a * n_lambda;
    const size_t at = ((size_t)a * n_groups + t) * n_lambda + l;
    l2[at] = (1.0 - mix[a]) * lambda[e];
    l1[at] = mix[a] * lambda[e];
    if (l == 0) ridge[(size_t)a * n_groups + t] = mix[a] == 0.0 ? 1 : 0;
  }
}

// One wavefront, the whole path.  Every lane computes the sweep's scalars (the new coefficient, the sweep's
// max|dw| and max|w|) from the same LDS words, so branches on them are uniform and nothing has to be broadcast.
// blockIdx.x = job; its training set is job % n_sets (M, scale and n per set), its penalties and outputs are the job's
// own.  One fit is a grid of 1 with n_sets = 1: n and the functor come as scalars (dn_sets = ridge_jobs = null).
__global__ __launch_bounds__(64) void cov_path_kernel(const double* __restrict__ M, const double* __restrict__ scale, int p, int n_sets,
                                                       double dn_one, const double* __restrict__ dn_sets,
                                                       const double* __restrict__ alpha, const double* __restrict__ beta, int n_lambda,
                                                       int ridge_one, const int32_t* __restrict__ ridge_jobs, unsigned max_iter, double tol,
                                                       double* __restrict__ W, double* __restrict__ G, double* __restrict__ c_out,
                                                       int32_t* __restrict__ sweeps_out, int32_t* __restrict__ unconverged) {
  __shared__ double lds[cov_state_doubles(kCovMaxFeatures)];
  const int lane = threadIdx.x, P1 = p + 1;
  const size_t job = blockIdx.x, set = job % (size_t)n_sets;
  M += set * (size_t)P1 * (size_t)P1;
  scale += set * (size_t)p;
  const double dn = dn_sets ? dn_sets[set] : dn_one;
  const int ridge = ridge_jobs ? ridge_jobs[job] : ridge_one;
  alpha += job * (size_t)n_lambda;
  beta += job * (size_t)n_lambda;
  W += job * (size_t)n_lambda * (size_t)p;
  G += job * (size_t)n_lambda * (size_t)p;
  c_out += job * (size_t)p;
  sweeps_out += job * (size_t)n_lambda;
  unconverged += job * (size_t)n_lambda;
  double* S = lds;
  double* c = S + p * (p + 1) / 2;
  double* w = c + p;
  double* g = w + p;
  for (int k = 0; k < p; ++k) {
    const double sk = scale[k];
    for (int j = lane; j <= k; j += 64) S[tri(j, k)] = M[(size_t)j * P1 + k] / dn / (scale[j] * sk);
  }
  for (int j = lane; j < p; j += 64) {
    c[j] = M[(size_t)j * P1 + p] / dn / scale[j];
    c_out[j] = c[j];
    w[j] = 0.0;
  }
  __syncthreads();
  for (int l = 0; l < n_lambda; ++l) {
    const double al = alpha[l], be = beta[l];
    // the gradient afresh at every lambda: what the incremental updates of the sweeps have rounded away does not
    // travel down the path
    for (int k = lane; k < p; k += 64) {
      double s = 0.0;
      for (int j = 0; j < p; ++j) s += S[j <= k ? tri(j, k) : tri(k, j)] * w[j];
      g[k] = s - c[k];
    }
    __syncthreads();
    unsigned sweeps = 0;
    bool converged = false;
    while (sweeps < max_iter && !converged) {
      double max_change = 0.0, max_size = 0.0;
      for (int j = 0; j < p; ++j) {
        const double wj = w[j], sjj = S[tri(j, j)];
        const double z = sjj * wj - g[j], denom = sjj + al;
        double nw = z;
        if (!ridge) nw = z > be ? z - be : (z < -be ? z + be : 0.0);
        nw = denom > 0.0 ? nw / denom : 0.0;       // a constant column without an l2 term: S_jj = c~_j = 0
        const double d = nw - wj;
        max_change = fmax(max_change, fabs(d));
        max_size = fmax(max_size, fabs(nw));
        if (d != 0.0) {
          __syncthreads();                         // every lane has read w[j] and g[j]
          if (lane == 0) w[j] = nw;
          for (int k = lane; k < p; k += 64) g[k] += S[k <= j ? tri(k, j) : tri(j, k)] * d;
          __syncthreads();
        }
      }
      ++sweeps;
      const bool all_zero = max_size == 0.0 && max_change == 0.0;
      const bool no_change = max_size != 0.0 && max_change / max_size <= tol;
      converged = all_zero || no_change;
    }
    for (int k = lane; k < p; k += 64) {
      W[(size_t)l * p + k] = w[k];
      G[(size_t)l * p + k] = g[k];
    }
    if (lane == 0) {
      sweeps_out[l] = (int32_t)sweeps;
      unconverged[l] = converged ? 0 : 1;
    }
  }
}

// The block update of feature j of cov_group_path_kernel, for one response: from the stored w_jr and g_jr to the new w_jr.
// scale = max(0, 1 - l1 / |z|) (1 for the ridge functor), 0 where |z| = 0 or the denominator is 0.  Every caller passes
// the same words through the same operations, so every lane holds the same bits.
__device__ __forceinline__ double group_new_w(double sjj, double wjr, double gjr, double shrink, double denom) {
  return shrink * fma(sjj, wjr, -gjr) / denom;
}

// Several responses (SGDNET_MODE_MCOVARIANCE): one workgroup of kWidth lanes, the whole path of
//   min  sum_r |y~_r - X~ w_r|^2 / (2 n) + l2 / 2 sum_jr w_jr^2 + l1 sum_j |w_j.|
// by cyclic block coordinate descent, a block the K coefficients of a feature.  S is shared by the responses; c~, w and
// g = S w - c~ are p x K, entry (j, r) at j K + r.  M is the (p + K) x (p + K) matrix of the moments pass.
// As in cov_path_kernel every lane computes |z|, the block's moves and the sweep's max|dw| and max|w| itself from the
// same LDS words in the same order (r = 0 .. K - 1): the branches around the barriers are uniform, nothing is broadcast,
// and a block that does not move costs no LDS write and no barrier.  A moving block: the lanes stride over the entries
// (k, r), k != j, of g and recompute the move d_r of their response from w_j. and g_j. (still the old ones: there is no
// room in the budget for K more doubles), then -- a barrier later -- row j of w and g is replaced: two barriers per
// moving block and one per sweep.
// blockIdx.x = job, as in cov_path_kernel: its training set is job % n_sets (rows j < p of M, scale and n per set), its
// penalties and outputs are the job's own.  One fit is a grid of 1 with n_sets = 1: n and the functor come as scalars
// (dn_sets = ridge_jobs = null).  The kernel declares the CU's whole LDS: one job runs per CU, the others queue.
template <int kWidth>
__global__ __launch_bounds__(kWidth) void cov_group_path_kernel(const double* __restrict__ M, const double* __restrict__ scale, int p, int K,
                                                                 int n_sets, double dn_one, const double* __restrict__ dn_sets,
                                                                 const double* __restrict__ alpha, const double* __restrict__ beta,
                                                                 int n_lambda, int ridge_one, const int32_t* __restrict__ ridge_jobs,
                                                                 unsigned max_iter, double tol, double* __restrict__ W,
                                                                 double* __restrict__ G, double* __restrict__ c_out,
                                                                 int32_t* __restrict__ sweeps_out, int32_t* __restrict__ unconverged) {
  __shared__ double lds[kCovLdsDoubles];
  const int lane = threadIdx.x, nc = p + K, pK = p * K;
  const size_t job = blockIdx.x, set = job % (size_t)n_sets;
  M += set * (size_t)p * (size_t)nc;
  scale += set * (size_t)p;
  const double dn = dn_sets ? dn_sets[set] : dn_one;
  const int ridge = ridge_jobs ? ridge_jobs[job] : ridge_one;
  alpha += job * (size_t)n_lambda;
  beta += job * (size_t)n_lambda;
  W += job * (size_t)n_lambda * (size_t)pK;
  G += job * (size_t)n_lambda * (size_t)pK;
  c_out += job * (size_t)pK;
  sweeps_out += job * (size_t)n_lambda;
  unconverged += job * (size_t)n_lambda;
  double* S = lds;
  double* c = S + p * (p + 1) / 2;
  double* w = c + pK;
  double* g = w + pK;
  for (int k = 0; k < p; ++k) {
    const double sk = scale[k];
    for (int j = lane; j <= k; j += kWidth) S[tri(j, k)] = M[(size_t)j * nc + k] / dn / (scale[j] * sk);
  }
  for (int e = lane; e < pK; e += kWidth) {
    const int j = e / K, r = e - j * K;
    c[e] = M[(size_t)j * nc + p + r] / dn / scale[j];
    c_out[e] = c[e];
    w[e] = 0.0;
  }
  __syncthreads();
  // the walk of a lane over the entries e = k K + r in strides of kWidth, without a division per entry
  const int k_first = lane / K, r_first = lane - k_first * K, k_step = kWidth / K, r_step = kWidth - k_step * K;
  for (int l = 0; l < n_lambda; ++l) {
    const double l2 = alpha[l], l1 = beta[l];
    // the gradient afresh at every lambda, as in cov_path_kernel
    for (int e = lane, k = k_first, r = r_first; e < pK; e += kWidth) {
      double s = 0.0;
      for (int j = 0; j < p; ++j) s += S[j <= k ? tri(j, k) : tri(k, j)] * w[j * K + r];
      g[e] = s - c[e];
      k += k_step;
      r += r_step;
      if (r >= K) {
        r -= K;
        ++k;
      }
    }
    __syncthreads();
    unsigned sweeps = 0;
    bool converged = false;
    while (sweeps < max_iter && !converged) {
      double max_change = 0.0, max_size = 0.0;
      for (int j = 0; j < p; ++j) {
        const double sjj = S[tri(j, j)], denom = sjj + l2;
        const double* wj = w + j * K;
        const double* gj = g + j * K;
        double zz = 0.0;
        for (int r = 0; r < K; ++r) {
          const double z = fma(sjj, wj[r], -gj[r]);
          zz = fma(z, z, zz);
        }
        const double nz = sqrt(zz);
        double shrink = 1.0;
        if (!ridge) shrink = nz > l1 ? 1.0 - l1 / nz : 0.0;
        if (!(nz > 0.0) || !(denom > 0.0)) shrink = 0.0;     // (a constant column without an l2 term: S_jj = c~_j. = 0)
        const double den = denom > 0.0 ? denom : 1.0;
        bool moved = false;
        for (int r = 0; r < K; ++r) {
          const double nw = group_new_w(sjj, wj[r], gj[r], shrink, den), d = nw - wj[r];
          max_change = fmax(max_change, fabs(d));
          max_size = fmax(max_size, fabs(nw));
          moved = moved || d != 0.0;
        }
        if (moved) {
          __syncthreads();                         // every lane has read what the blocks that stayed needed
          for (int e = lane, k = k_first, r = r_first; e < pK; e += kWidth) {
            if (k != j) {
              const double d = group_new_w(sjj, wj[r], gj[r], shrink, den) - wj[r];
              g[e] = fma(S[k <= j ? tri(k, j) : tri(j, k)], d, g[e]);
            }
            k += k_step;
            r += r_step;
            if (r >= K) {
              r -= K;
              ++k;
            }
          }
          __syncthreads();                         // every lane has read the old w_j. and g_j.
          for (int r = lane; r < K; r += kWidth) {
            const double nw = group_new_w(sjj, wj[r], gj[r], shrink, den), d = nw - wj[r];
            g[j * K + r] = fma(sjj, d, gj[r]);
            w[j * K + r] = nw;
          }
          // (row j is read again by the next sweep, or by the copy out: behind the sweep's barrier.  Until then a later
          //  block reads its own row, which the loop above finished before the barrier, and writes behind its first one)
        }
      }
      __syncthreads();
      ++sweeps;
      const bool all_zero = max_size == 0.0 && max_change == 0.0;
      const bool no_change = max_size != 0.0 && max_change / max_size <= tol;
      converged = all_zero || no_change;
    }
    for (int e = lane; e < pK; e += kWidth) {
      W[(size_t)l * pK + e] = w[e];
      G[(size_t)l * pK + e] = g[e];
    }
    if (lane == 0) {
      sweeps_out[l] = (int32_t)sweeps;
      unconverged[l] = converged ? 0 : 1;
    }
  }
}

// The path kernel's workgroup.  Both widths give the same bits (every entry is updated by one lane from the same words in
// the same order); profiles/mcovariance_path.txt has their times: at 300 x 174, K = 10 four wavefronts halve the path
// (284 -> 137 ms), at 4000 x 9, K = 3 (27 entries) three of them would only wait at the barriers (1.30 -> 1.36 ms).
// So: one wavefront while one stride of it covers all p K entries, four beyond.
constexpr int kMcovNarrow = 64, kMcovWide = 256;
constexpr int mcov_path_width(size_t entries) { return entries <= (size_t)kMcovNarrow ? kMcovNarrow : kMcovWide; }

// ---- wide covariance mode (SGDNET_MODE_WCOVARIANCE): S in global memory, only what can move is touched ----

// The coordinate update of cov_wide_path_kernel, for the screen (w_j = 0) and for the sweep: from S_jj, w_j and g_j to the
// new w_j.  Every caller passes the same words through the same operations, so every lane holds the same bits.
__device__ __forceinline__ double cov_coord_new_w(double sjj, double wj, double gj, double al, double be, int ridge) {
  const double z = fma(sjj, wj, -gj), denom = sjj + al;
  double nw = z;
  if (!ridge) nw = z > be ? z - be : (z < -be ? z + be : 0.0);
  return denom > 0.0 ? nw / denom : 0.0;          // a constant column without an l2 term: S_jj = c~_j = 0
}

// One workgroup of kWidth lanes, the whole path, S (leading dimension ld, a multiple of 16) read from global memory.
// LDS (covariance.hpp: wcov_state_bytes): g | c~ | w | diag S | the list | the list's bits | the compaction's counts.
// Per lambda, warm-started:
//   rebuild  the list becomes {j : w_j != 0}, ascending; g = sum_{j in list} S[:, j] w_j - c~ afresh (a lane owns two
//            consecutive k, j ascends: one 16-byte load per column, four columns requested before the first is used)
//   screen   every j outside the list: the coordinate update from w_j = 0; those that would move join.  The list is
//            compacted again from its bits (wide_cd_device.hpp: wide_compact)
//   sweep    cov_path_kernel's cyclic coordinate descent over the list: every lane computes the scalars from the same LDS
//            words (uniform branches); a coordinate that stays costs no global read and no barrier; one that moves by d
//            does g[k] += S[k, j] d for ALL k < p (so g stays the full gradient and the screen needs no pass over S),
//            16 bytes a lane.  The reference's ConvergenceCheck over the list ends the sweeps; then the screen runs
//            again, and the lambda is done when it adds nothing.
// max_iter bounds the list sweeps of one lambda.  g[k] is updated by one lane from the same words in the same order
// whatever kWidth is: both widths give the same bits.
// The body of two entries, below: cov_wide_path_kernel (one fit) and cov_wide_cv_path_kernel (a job of a cross-validation).
template <int kWidth, bool kPrefetch>
__device__ __forceinline__ void cov_wide_path_body(const double* __restrict__ S, const double* __restrict__ Sd,
                                                   const double* __restrict__ ct, int p, int ld,
                                                   const double* __restrict__ alpha, const double* __restrict__ beta,
                                                   int n_lambda, int ridge, unsigned max_iter, double tol,
                                                   double* __restrict__ W, double* __restrict__ G,
                                                   int32_t* __restrict__ sweeps_out, int32_t* __restrict__ unconverged) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[kCovLdsBytes];
  const int lane = threadIdx.x;
  double* g = reinterpret_cast<double*>(lds);
  double* c = g + p;
  double* w = c + p;
  double* sd = w + p;
  int32_t* list = reinterpret_cast<int32_t*>(sd + p);
  uint32_t* bits = reinterpret_cast<uint32_t*>(list + p);
  int32_t* counts = reinterpret_cast<int32_t*>(bits + (p + 31) / 32);
  const int slots = (p + 1) / 2;     // a slot: k = 2 s and 2 s + 1 (p odd: the last one's second entry is S's zero pad)
  // kPrefetch: a lane's slots of one column of S, requested while the move before it updates g (S never changes, so
  // what is held stays valid until the sweep reaches column held_j, in this sweep or a later one)
  constexpr int kSlots = ((kWcovMaxFeatures + 1) / 2 + kWidth - 1) / kWidth, kLookAhead = 8;
  double2 held[kSlots];
  int held_j = -1;
  auto fetch = [&](int j, double2(&buf)[kSlots]) {
    const double* col = S + (size_t)ld * j;
#pragma unroll
    for (int u = 0; u < kSlots; ++u) {
      const int s = lane + u * kWidth;
      if (s < slots) buf[u] = *reinterpret_cast<const double2*>(col + 2 * s);
    }
  };
  for (int j = lane; j < p; j += kWidth) {
    c[j] = ct[j];
    sd[j] = Sd[j];
    w[j] = 0.0;
  }
  __syncthreads();

  // The list from one flag per coordinate (wide_cd_device.hpp: wide_compact).  screen: the flag is "in the list already,
  // or would move from 0"; else: w_j != 0.  (One functor with a run-time `screen` and its own j < p, not one per call site:
  // in this shape the kernel compiles to the instructions it had with its own copy of the compaction.)
  auto compact = [&](bool screen, double al, double be) -> int {
    return wide_compact<kWidth>(p, list, bits, counts, [&](int j) -> bool {
      bool in = false;
      if (j < p) {
        if (screen) {
          in = (bits[j >> 5] >> (j & 31)) & 1u;
          if (!in) in = cov_coord_new_w(sd[j], 0.0, g[j], al, be, ridge) != 0.0;
        } else {
          in = w[j] != 0.0;
        }
      }
      return in;
    });
  };

  for (int l = 0; l < n_lambda; ++l) {
    const double al = alpha[l], be = beta[l];
    int n_list = compact(false, al, be);
    // the gradient afresh at every lambda, as in cov_path_kernel
    for (int s = lane; s < slots; s += kWidth) {
      const int k = 2 * s;
      const double* col = S + k;
      double a0 = 0.0, a1 = 0.0;
      int i = 0;
      for (; i + 4 <= n_list; i += 4) {
        const int j0 = list[i], j1 = list[i + 1], j2 = list[i + 2], j3 = list[i + 3];
        const double2 v0 = *reinterpret_cast<const double2*>(col + (size_t)ld * j0);
        const double2 v1 = *reinterpret_cast<const double2*>(col + (size_t)ld * j1);
        const double2 v2 = *reinterpret_cast<const double2*>(col + (size_t)ld * j2);
        const double2 v3 = *reinterpret_cast<const double2*>(col + (size_t)ld * j3);
        const double w0 = w[j0], w1 = w[j1], w2 = w[j2], w3 = w[j3];
        a0 = fma(v0.x, w0, a0);
        a1 = fma(v0.y, w0, a1);
        a0 = fma(v1.x, w1, a0);
        a1 = fma(v1.y, w1, a1);
        a0 = fma(v2.x, w2, a0);
        a1 = fma(v2.y, w2, a1);
        a0 = fma(v3.x, w3, a0);
        a1 = fma(v3.y, w3, a1);
      }
      for (; i < n_list; ++i) {
        const int j = list[i];
        const double2 v = *reinterpret_cast<const double2*>(col + (size_t)ld * j);
        a0 = fma(v.x, w[j], a0);
        a1 = fma(v.y, w[j], a1);
      }
      g[k] = a0 - c[k];
      if (k + 1 < p) g[k + 1] = a1 - c[k + 1];
    }
    __syncthreads();

    unsigned sweeps = 0;
    bool converged = false;
    for (int screens = 0;; ++screens) {
      const int n_new = compact(true, al, be);
      if (screens > 0 && n_new == n_list) {      // the list had converged and nothing outside it moves
        converged = true;
        break;
      }
      n_list = n_new;
      bool met = false;
      while (sweeps < max_iter && !met) {
        double max_change = 0.0, max_size = 0.0;
        for (int i = 0; i < n_list; ++i) {
          const int j = list[i];
          const double wj = w[j];
          const double nw = cov_coord_new_w(sd[j], wj, g[j], al, be, ridge);
          const double d = nw - wj;
          max_change = fmax(max_change, fabs(d));
          max_size = fmax(max_size, fabs(nw));
          if (d != 0.0 && kPrefetch) {
            // the column of this move: the one held, or fetched now; then the request for the next entry of the list
            // (at most kLookAhead on, wrapping to the next sweep) whose coefficient is not 0: the likeliest to move
            double2 now[kSlots];
            if (held_j == j) {
#pragma unroll
              for (int u = 0; u < kSlots; ++u) now[u] = held[u];
            } else {
              fetch(j, now);
            }
            held_j = -1;
            for (int t = 1; t <= kLookAhead && t < n_list && held_j < 0; ++t) {
              const int next = list[i + t < n_list ? i + t : i + t - n_list];
              if (w[next] != 0.0) held_j = next;
            }
            if (held_j >= 0) fetch(held_j, held);
            __syncthreads();                         // every lane has read w[j] and g[j]
            if (lane == 0) w[j] = nw;
#pragma unroll
            for (int u = 0; u < kSlots; ++u) {
              const int k = 2 * (lane + u * kWidth);
              if (k + 1 < p) {
                double2 gk = *reinterpret_cast<double2*>(g + k);
                gk.x = fma(now[u].x, d, gk.x);
                gk.y = fma(now[u].y, d, gk.y);
                *reinterpret_cast<double2*>(g + k) = gk;
              } else if (k < p) {
                g[k] = fma(now[u].x, d, g[k]);
              }
            }
            __syncthreads();
          } else if (d != 0.0) {
            __syncthreads();                         // every lane has read w[j] and g[j]
            if (lane == 0) w[j] = nw;
            wide_column_move<kWidth>(g, S + (size_t)ld * j, p, d);
            __syncthreads();
          }
        }
        ++sweeps;
        const bool all_zero = max_size == 0.0 && max_change == 0.0;
        const bool no_change = max_size != 0.0 && max_change / max_size <= tol;
        met = all_zero || no_change;
      }
      if (!met) break;                               // max_iter
    }
    for (int k = lane; k < p; k += kWidth) {
      W[(size_t)l * p + k] = w[k];
      G[(size_t)l * p + k] = g[k];
    }
    if (lane == 0) {
      sweeps_out[l] = (int32_t)sweeps;
      unconverged[l] = converged ? 0 : 1;
    }
  }
}

// One fit: a grid of 1.  The entry the single fit has always had, around the shared body.
template <int kWidth, bool kPrefetch>
__global__ __launch_bounds__(kWidth) void cov_wide_path_kernel(const double* __restrict__ S, const double* __restrict__ Sd,
                                                                const double* __restrict__ ct, int p, int ld,
                                                                const double* __restrict__ alpha, const double* __restrict__ beta,
                                                                int n_lambda, int ridge, unsigned max_iter, double tol,
                                                                double* __restrict__ W, double* __restrict__ G,
                                                                int32_t* __restrict__ sweeps_out, int32_t* __restrict__ unconverged) {
  cov_wide_path_body<kWidth, kPrefetch>(S, Sd, ct, p, ld, alpha, beta, n_lambda, ridge, max_iter, tol, W, G, sweeps_out, unconverged);
}

// The same path over jobs (wcovariance_cv_run).  blockIdx.x = job, as in cov_path_kernel: its training set is job % n_sets
// (S, diag S and c~ per set: strides ld p, p and p; a set's S is read-only and shared by its mixes), its penalties, functor
// and outputs are the job's own.  The pointers are offset once, here at the entry, and the body is the single fit's: a
// second entry rather than more arguments to the first, because with the job's arguments the single fit's <1024, ahead>
// instance took one more VGPR (profiles/cv_wcovariance.txt has the registers of all eight).  The kernel declares the
// CU's whole LDS: one job runs per CU, the others queue.
template <int kWidth, bool kPrefetch>
__global__ __launch_bounds__(kWidth) void cov_wide_cv_path_kernel(const double* __restrict__ S, const double* __restrict__ Sd,
                                                                   const double* __restrict__ ct, int p, int ld, int n_sets,
                                                                   const double* __restrict__ alpha, const double* __restrict__ beta,
                                                                   int n_lambda, const int32_t* __restrict__ ridge_jobs,
                                                                   unsigned max_iter, double tol, double* __restrict__ W,
                                                                   double* __restrict__ G, int32_t* __restrict__ sweeps_out,
                                                                   int32_t* __restrict__ unconverged) {
  const size_t job = blockIdx.x, set = job % (size_t)n_sets, at = job * (size_t)n_lambda;
  cov_wide_path_body<kWidth, kPrefetch>(S + set * (size_t)ld * (size_t)p, Sd + set * (size_t)p, ct + set * (size_t)p, p, ld, alpha + at,
                                        beta + at, n_lambda, ridge_jobs[job], max_iter, tol, W + at * (size_t)p, G + at * (size_t)p,
                                        sweeps_out + at, unconverged + at);
}

// The wide path kernel's workgroup and whether it requests the next column ahead: all four instances give the same bits;
// profiles/wcovariance_path.txt has the path kernel's time for each at p = 198, 1000, 2000 and 4000 (100 lambdas):
//   lanes, ahead      p = 198     1000     2000     4000
//   256,  no           8.3 ms     85 ms   499 ms   830 ms
//   1024, no          10.4 ms     82 ms   227 ms   340 ms
//   256,  yes         16.1 ms    103 ms   257 ms   320 ms
//   1024, yes         14.2 ms     83 ms   218 ms   255 ms
// A column of 198 doubles is less than one stride of 256 lanes, and twelve more wavefronts only wait at the barriers;
// from 1000 on the sixteen wavefronts win.  Looking ahead costs a scan of the list and a copy of the held registers per
// move: it loses where a column comes back from L2 at once and wins (4 % at 2000, 25 % at 4000) where a move waits for
// its column.  So: 256 lanes up to 512 features, 1024 beyond (wide_layout.hpp: wide_cd_width); ahead beyond 1536 (between
// the two measurements).
constexpr bool wcov_path_ahead(int p) { return p > 1536; }

// ---- the folds of wide covariance mode (wcovariance_cv_run): cov_assemble_kernel's work, written in the wide layout ----
// cov_assemble_kernel is one workgroup per training set with the sums s and the shifts d in static LDS sized for 198
// features; at 4531 features a set's matrix is 20 M entries and the two vectors 72.5 KB.  So the work is cut in two, and s
// and d live in GLOBAL memory (2 G (p + 1) doubles, read through L2 by the second kernel; no dynamic LDS, no attribute):
//   wcov_cv_stats_kernel     blockIdx.x = training set T: everything of size p or smaller
//   wcov_cv_assemble_kernel  blockIdx.x = column j, blockIdx.y = T: column j of S_T, diag S_T and c~_T
// No G x (p + 1)^2 re-centred matrix is written in between: a column of S_T comes straight from row j of the group moments.

// The (p + 2) x (p + 2) moments of training set T about the common centre: group T alone, or (rest) the total less group T.
struct WcovSet {
  const double* Ct;
  const double* total;
  int Pa, rest;
  __device__ __forceinline__ double operator()(int j, int k) const {
    const double v = Ct[(size_t)j * Pa + k];
    return rest ? total[(size_t)j * Pa + k] - v : v;
  }
  // the magnitude its rounding is relative to (cov_constant_on_set)
  __device__ __forceinline__ double magnitude(int j, int k) const {
    const double v = fabs(Ct[(size_t)j * Pa + k]);
    return rest ? fabs(total[(size_t)j * Pa + k]) + v : v;
  }
};

// cov_assemble_kernel's re-centring of entry (j, k), j <= k, from the entry c about the common centre, T's sums of deviations
// s and its shifts d: the operands come in the order of the smaller index first, so that (j, k) and (k, j) give the same bits
// (the moments are symmetric bit for bit: cov_reduce_kernel and cov_sparse_pair_kernel store every entry twice)
__device__ __forceinline__ double wcov_recentred(double c, double sj, double dj, double sk, double dk, double nT) {
  return c - dj * sk - dk * sj + nT * dj * dk;
}

// blockIdx.x = training set T.  From the group moments to what is per T or per job and of size p or smaller, as
// cov_assemble_kernel leaves it (the same expressions):
//   s, d   G x (p + 1): T's sums of deviations about the common centre and its shifts d = t - a (0 where not centred)
//   cst    G x (p + 1): the column is constant on T (cov_constant_on_set): scale 1, zeros in S_T and c~_T
//   scale  G x p      mean  G x (p + 1): t (0 where the features are not centred), mean_T(y)
//   tstat  3 x G: n_T | sd_T(y) (0 -> 1) | y~'y~         alpha, beta  jobs x n_lambda, job = mix * G + T      ridge  jobs
// Every lane computes sd_T(y) itself from the same four words: nothing is staged and no barrier is needed.
__global__ __launch_bounds__(kBlock) void wcov_cv_stats_kernel(const double* __restrict__ Mg, const double* __restrict__ total,
                                                                const double* __restrict__ mu, int n_groups, int p, int rest, int centre,
                                                                int standardize, const double* __restrict__ mix,
                                                                const double* __restrict__ lambda, int n_mix, int n_lambda,
                                                                double* __restrict__ s, double* __restrict__ d, int32_t* __restrict__ cst,
                                                                double* __restrict__ scale, double* __restrict__ mean,
                                                                double* __restrict__ tstat, double* __restrict__ alpha,
                                                                double* __restrict__ beta, int32_t* __restrict__ ridge) {
  const int t = blockIdx.x, tid = threadIdx.x, P1 = p + 1, Pa = p + 2;
  const WcovSet C{Mg + (size_t)t * Pa * Pa, total, Pa, rest};
  const int n_summed = rest ? n_groups : 0;
  const double nT = C(p + 1, p + 1);
  const double sy = C(p, p + 1), dy = sy / nT;
  const double qy = wcov_recentred(C(p, p), sy, dy, sy, dy, nT);
  const bool cst_y = cov_constant_on_set(qy, C.magnitude(p, p), C.magnitude(p, p + 1), dy, nT, n_summed);
  const double sd_y = cst_y ? 1.0 : sqrt(qy / nT);
  for (int j = tid; j < P1; j += kBlock) {
    const double sj = C(j, p + 1), dj = (j == p || centre) ? sj / nT : 0.0;
    s[(size_t)t * P1 + j] = sj;
    d[(size_t)t * P1 + j] = dj;
    const double q = wcov_recentred(C(j, j), sj, dj, sj, dj, nT);
    const bool cj = cov_constant_on_set(q, C.magnitude(j, j), C.magnitude(j, p + 1), dj, nT, n_summed);
    cst[(size_t)t * P1 + j] = cj ? 1 : 0;
    if (j < p) {
      scale[(size_t)t * p + j] = (standardize && !cj) ? sqrt(q / nT) : 1.0;
      mean[(size_t)t * P1 + j] = centre ? mu[j] + dj : 0.0;
    }
  }
  if (tid == 0) {
    mean[(size_t)t * P1 + p] = mu[p + 1] + dy;
    tstat[t] = nT;
    tstat[n_groups + t] = sd_y;
    tstat[2 * n_groups + t] = cst_y ? 0.0 : qy / sd_y / sd_y;
  }
  for (int e = tid; e < n_mix * n_lambda; e += kBlock) {
    const int a = e / n_lambda, l = e - a * n_lambda;
    const size_t at = ((size_t)a * n_groups + t) * n_lambda + l;
    alpha[at] = (1.0 - mix[a]) * lambda[e] / sd_y;
    beta[at] = mix[a] * lambda[e] / sd_y;
    if (l == 0) ridge[(size_t)a * n_groups + t] = mix[a] == 0.0 ? 1 : 0;
  }
}

// blockIdx.x = column j < p, blockIdx.y = training set T.  Column j of S_T = M^T / n_T / (sd sd') in the layout
// cov_wide_path_kernel reads (leading dimension ld, rows p .. ld - 1 the zero pad; set stride ld p), diag S_T and
// c~_T,j = M^T[j, y] / sd_T(y) / n_T / sd_j: the arithmetic of cov_assemble_kernel followed by wide_scale_kernel's.  The
// moments are read along row j (coalesced; row j is column j bit for bit); s, d and scale come from wcov_cv_stats_kernel.
__global__ __launch_bounds__(kBlock) void wcov_cv_assemble_kernel(const double* __restrict__ Mg, const double* __restrict__ total,
                                                                   const double* __restrict__ s, const double* __restrict__ d,
                                                                   const int32_t* __restrict__ cst, const double* __restrict__ scale,
                                                                   const double* __restrict__ tstat, int n_groups, int p, int ld, int rest,
                                                                   double* __restrict__ S, double* __restrict__ Sd, double* __restrict__ ct) {
  const int j = blockIdx.x, t = blockIdx.y, P1 = p + 1, Pa = p + 2;
  const WcovSet C{Mg + (size_t)t * Pa * Pa, total, Pa, rest};
  s += (size_t)t * P1;
  d += (size_t)t * P1;
  cst += (size_t)t * P1;
  scale += (size_t)t * p;
  const double nT = tstat[t], sd_y = tstat[n_groups + t];
  const double sj = s[j], dj = d[j], fj = scale[j];
  const bool cj = cst[j] != 0;
  double* col = S + ((size_t)t * p + j) * (size_t)ld;
  for (int k = threadIdx.x; k < ld; k += kBlock) {
    double v = 0.0;
    if (k < p && !cj && !cst[k]) {
      const double c = C(j, k), sk = s[k], dk = d[k], fk = scale[k];
      v = k >= j ? wcov_recentred(c, sj, dj, sk, dk, nT) / nT / (fj * fk) : wcov_recentred(c, sk, dk, sj, dj, nT) / nT / (fk * fj);
    }
    col[k] = v;
    if (k == j) Sd[(size_t)t * p + j] = v;
  }
  if (threadIdx.x == 0) ct[(size_t)t * p + j] = (cj || cst[p]) ? 0.0 : wcov_recentred(C(j, p), sj, dj, s[p], d[p], nT) / sd_y / nT / fj;
}

// ---- wide multi-response mode (SGDNET_MODE_WMCOVARIANCE): cov_group_path_kernel's problem, S in global memory ----

// wide_scale_kernel for K right-hand sides.  blockIdx.x = feature j: column j of S (leading dimension ld, rows p .. ld - 1
// the zero pad) and diag S from the upper triangle of the (p + K) x (p + K) moment matrix M, and rhs_jr = M[j, p + r] / n / s_j
// at j K + r: the arithmetic of cov_group_path_kernel's prologue.
__global__ __launch_bounds__(kBlock) void cov_wide_group_scale_kernel(const double* __restrict__ M, const double* __restrict__ scale, int p,
                                                                       int K, int ld, double dn, double* __restrict__ A,
                                                                       double* __restrict__ Ad, double* __restrict__ rhs) {
  const int j = blockIdx.x, nc = p + K;
  const double sj = scale[j];
  for (int k = threadIdx.x; k < ld; k += kBlock) {
    double v = 0.0;
    if (k < p) {
      const double sk = scale[k];
      v = k >= j ? M[(size_t)j * nc + k] / dn / (sj * sk) : M[(size_t)k * nc + j] / dn / (sk * sj);
    }
    A[(size_t)j * ld + k] = v;
    if (k == j) Ad[j] = v;
  }
  for (int r = threadIdx.x; r < K; r += kBlock) rhs[(size_t)j * K + r] = M[(size_t)j * nc + p + r] / dn / sj;
}

// One workgroup of kWidth lanes, the whole path of cov_group_path_kernel's problem, S (leading dimension ld, a multiple of
// 16) and c~ (p x K, entry (j, r) at j K + r) read from global memory.
// LDS (covariance.hpp: wmcov_state_bytes): g | w | diag S | a block's new coefficients | the list | its bits | the counts.
// g and w are response-major: entry (k, r) at r pe + k, pe = p rounded up to even, so that the slot (2 s, 2 s + 1) of the
// column move is 16 bytes and aligned in every response; the pad entry of an odd p meets S's zero pad and stays 0.
// c~ is not in LDS: it is read once per lambda, by the rebuild.
// Per lambda, warm-started, cov_wide_path_kernel's phases with a block (the K coefficients of a feature) for a coordinate:
//   rebuild  the list becomes {j : w_j. != 0}, ascending; g = sum_{j in list} S[:, j] w_j. - c~ afresh (a lane owns the
//            slots of two consecutive k in all K responses, j ascends: one 16-byte load of a column serves the K responses,
//            four columns requested before the first is used)
//   screen   every j outside the list (w_j. = 0): cov_group_path_kernel's block update; the blocks that would move join
//            (|g_j.| > l1; ridge: g_j. != 0 and S_jj + l2 > 0).  The list is compacted again from its bits (wide_compact)
//   sweep    cyclic block coordinate descent over the list with the arithmetic of group_new_w.  Every lane computes |z|,
//            the shrink, the K moves and the sweep's max|dw| and max|w| itself from the same LDS words in the order
//            r = 0 .. K - 1: the branches around the barriers are uniform, and a block that stays costs no global read
//            and no barrier.  A block that moves: lane r leaves the new w_jr in the K doubles of scratch; a barrier; every
//            lane does g[k, r] += S[k, j] (new w_jr - w_jr) for its slots and all r -- ALL k < p, row j included, so g stays
//            the full gradient; a barrier; lane r puts the new w_jr in place (read again behind the sweep's barrier only).
//            Two barriers per moving block and one per sweep.  The reference's ConvergenceCheck over the list ends the
//            sweeps; then the screen runs again, and the lambda is done when it adds nothing.
// max_iter bounds the list sweeps of one lambda.  Every entry of g is updated by one lane from the same words in the same
// order whatever kWidth is: both widths give the same bits.
// The body of two entries, below: cov_wide_group_path_kernel (one fit) and cov_wide_group_cv_path_kernel (a job of a
// cross-validation).
template <int kWidth>
__device__ __forceinline__ void cov_wide_group_path_body(const double* __restrict__ S, const double* __restrict__ Sd,
                                                         const double* __restrict__ ct, int p, int K, int ld,
                                                         const double* __restrict__ alpha, const double* __restrict__ beta,
                                                         int n_lambda, int ridge, unsigned max_iter, double tol,
                                                         double* __restrict__ W, double* __restrict__ G,
                                                         int32_t* __restrict__ sweeps_out, int32_t* __restrict__ unconverged) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[kCovLdsBytes];
  const int lane = threadIdx.x, pe = p + (p & 1), slots = pe / 2, pK = p * K;
  double* g = reinterpret_cast<double*>(lds);
  double* w = g + K * pe;
  double* sd = w + K * pe;
  double* moved_to = sd + p;
  int32_t* list = reinterpret_cast<int32_t*>(moved_to + K);
  uint32_t* bits = reinterpret_cast<uint32_t*>(list + p);
  int32_t* counts = reinterpret_cast<int32_t*>(bits + (p + 31) / 32);
  for (int e = lane; e < 2 * K * pe; e += kWidth) g[e] = 0.0;        // g and w, their pads included
  for (int j = lane; j < p; j += kWidth) sd[j] = Sd[j];
  __syncthreads();

  // the shrink and the denominator of block j from the stored w_j. and g_j., as cov_group_path_kernel forms them
  auto block_shrink = [&](int j, double sjj, double l1, double l2, double* den) -> double {
    double zz = 0.0;
    for (int r = 0; r < K; ++r) {
      const double z = fma(sjj, w[r * pe + j], -g[r * pe + j]);
      zz = fma(z, z, zz);
    }
    const double nz = sqrt(zz), denom = sjj + l2;
    double shrink = 1.0;
    if (!ridge) shrink = nz > l1 ? 1.0 - l1 / nz : 0.0;
    if (!(nz > 0.0) || !(denom > 0.0)) shrink = 0.0;     // (a constant column without an l2 term: S_jj = c~_j. = 0)
    *den = denom > 0.0 ? denom : 1.0;
    return shrink;
  };

  // The list from one flag per block (wide_cd_device.hpp: wide_compact).  screen: the flag is "in the list already, or
  // would move" (a block outside the list has w_j. = 0); else: w_j. != 0.
  auto compact = [&](bool screen, double l1, double l2) -> int {
    return wide_compact<kWidth>(p, list, bits, counts, [&](int j) -> bool {
      bool in = false;
      if (j < p) {
        if (screen) {
          in = (bits[j >> 5] >> (j & 31)) & 1u;
          if (!in) {
            double den;
            const double sjj = sd[j], shrink = block_shrink(j, sjj, l1, l2, &den);
            if (shrink != 0.0)
              for (int r = 0; r < K && !in; ++r) in = group_new_w(sjj, w[r * pe + j], g[r * pe + j], shrink, den) != 0.0;
          }
        } else {
          for (int r = 0; r < K && !in; ++r) in = w[r * pe + j] != 0.0;
        }
      }
      return in;
    });
  };

  // g[k .. k + 1, r] += v w_jr for all r: a column's slot applied to the K responses (the rebuild)
  auto add_column = [&](int k, double2 v, int j) {
    for (int r = 0; r < K; ++r) {
      const double wjr = w[r * pe + j];
      double2 gk = *reinterpret_cast<double2*>(g + r * pe + k);
      gk.x = fma(v.x, wjr, gk.x);
      gk.y = fma(v.y, wjr, gk.y);
      *reinterpret_cast<double2*>(g + r * pe + k) = gk;
    }
  };

  for (int l = 0; l < n_lambda; ++l) {
    const double l2 = alpha[l], l1 = beta[l];
    int n_list = compact(false, l1, l2);
    // the gradient afresh at every lambda, as in cov_path_kernel
    for (int s = lane; s < slots; s += kWidth) {
      const int k = 2 * s;
      for (int r = 0; r < K; ++r) *reinterpret_cast<double2*>(g + r * pe + k) = make_double2(0.0, 0.0);
      const double* col = S + k;
      int i = 0;
      for (; i + 4 <= n_list; i += 4) {
        const int j0 = list[i], j1 = list[i + 1], j2 = list[i + 2], j3 = list[i + 3];
        const double2 v0 = *reinterpret_cast<const double2*>(col + (size_t)ld * j0);
        const double2 v1 = *reinterpret_cast<const double2*>(col + (size_t)ld * j1);
        const double2 v2 = *reinterpret_cast<const double2*>(col + (size_t)ld * j2);
        const double2 v3 = *reinterpret_cast<const double2*>(col + (size_t)ld * j3);
        add_column(k, v0, j0);
        add_column(k, v1, j1);
        add_column(k, v2, j2);
        add_column(k, v3, j3);
      }
      for (; i < n_list; ++i) {
        const int j = list[i];
        add_column(k, *reinterpret_cast<const double2*>(col + (size_t)ld * j), j);
      }
      for (int r = 0; r < K; ++r) {
        g[r * pe + k] -= ct[(size_t)k * K + r];
        if (k + 1 < p) g[r * pe + k + 1] -= ct[(size_t)(k + 1) * K + r];
      }
    }
    __syncthreads();

    unsigned sweeps = 0;
    bool converged = false;
    for (int screens = 0;; ++screens) {
      const int n_new = compact(true, l1, l2);
      if (screens > 0 && n_new == n_list) {      // the list had converged and nothing outside it moves
        converged = true;
        break;
      }
      n_list = n_new;
      bool met = false;
      while (sweeps < max_iter && !met) {
        double max_change = 0.0, max_size = 0.0;
        for (int i = 0; i < n_list; ++i) {
          const int j = list[i];
          const double sjj = sd[j];
          double den;
          const double shrink = block_shrink(j, sjj, l1, l2, &den);
          bool moved = false;
          for (int r = 0; r < K; ++r) {
            const double wjr = w[r * pe + j];
            const double nw = group_new_w(sjj, wjr, g[r * pe + j], shrink, den), d = nw - wjr;
            max_change = fmax(max_change, fabs(d));
            max_size = fmax(max_size, fabs(nw));
            moved = moved || d != 0.0;
          }
          if (moved) {
            for (int r = lane; r < K; r += kWidth) moved_to[r] = group_new_w(sjj, w[r * pe + j], g[r * pe + j], shrink, den);
            __syncthreads();                         // every lane has read w_j. and g_j.; the new w_j. is in the scratch
            const double* col = S + (size_t)ld * j;
            for (int s = lane; s < slots; s += kWidth) {
              const int k = 2 * s;
              const double2 v = *reinterpret_cast<const double2*>(col + k);
              for (int r = 0; r < K; ++r) {
                const double d = moved_to[r] - w[r * pe + j];
                double2 gk = *reinterpret_cast<double2*>(g + r * pe + k);
                gk.x = fma(v.x, d, gk.x);
                gk.y = fma(v.y, d, gk.y);
                *reinterpret_cast<double2*>(g + r * pe + k) = gk;
              }
            }
            __syncthreads();                         // every lane has read the old w_j.
            for (int r = lane; r < K; r += kWidth) w[r * pe + j] = moved_to[r];
            // (row j of w is read again by the next sweep, by a screen or by the copy out: behind the sweep's barrier.
            //  The scratch entry r is lane r's own, so the next moving block overwrites it behind this read)
          }
        }
        __syncthreads();
        ++sweeps;
        const bool all_zero = max_size == 0.0 && max_change == 0.0;
        const bool no_change = max_size != 0.0 && max_change / max_size <= tol;
        met = all_zero || no_change;
      }
      if (!met) break;                               // max_iter
    }
    for (int e = lane; e < pK; e += kWidth) {
      const int j = e / K, r = e - j * K;
      W[(size_t)l * pK + e] = w[r * pe + j];
      G[(size_t)l * pK + e] = g[r * pe + j];
    }
    if (lane == 0) {
      sweeps_out[l] = (int32_t)sweeps;
      unconverged[l] = converged ? 0 : 1;
    }
  }
}

// One fit: a grid of 1.  The entry the single fit has always had, around the shared body.
template <int kWidth>
__global__ __launch_bounds__(kWidth) void cov_wide_group_path_kernel(const double* __restrict__ S, const double* __restrict__ Sd,
                                                                      const double* __restrict__ ct, int p, int K, int ld,
                                                                      const double* __restrict__ alpha, const double* __restrict__ beta,
                                                                      int n_lambda, int ridge, unsigned max_iter, double tol,
                                                                      double* __restrict__ W, double* __restrict__ G,
                                                                      int32_t* __restrict__ sweeps_out, int32_t* __restrict__ unconverged) {
  cov_wide_group_path_body<kWidth>(S, Sd, ct, p, K, ld, alpha, beta, n_lambda, ridge, max_iter, tol, W, G, sweeps_out, unconverged);
}

// The same path over jobs (wmcovariance_cv_run).  blockIdx.x = job, as in cov_wide_cv_path_kernel: its training set is
// job % n_sets (S, diag S and c~ per set: strides ld p, p and p K; read-only and shared by the set's mixes), its penalties,
// functor and outputs are the job's own.  The pointers are offset once, here at the entry, and the body is the single
// fit's; a second entry for the reason cov_wide_cv_path_kernel is one.  The kernel declares the CU's whole LDS: one job
// runs per CU, the others queue.
template <int kWidth>
__global__ __launch_bounds__(kWidth) void cov_wide_group_cv_path_kernel(const double* __restrict__ S, const double* __restrict__ Sd,
                                                                         const double* __restrict__ ct, int p, int K, int ld, int n_sets,
                                                                         const double* __restrict__ alpha, const double* __restrict__ beta,
                                                                         int n_lambda, const int32_t* __restrict__ ridge_jobs,
                                                                         unsigned max_iter, double tol, double* __restrict__ W,
                                                                         double* __restrict__ G, int32_t* __restrict__ sweeps_out,
                                                                         int32_t* __restrict__ unconverged) {
  const size_t job = blockIdx.x, set = job % (size_t)n_sets, at = job * (size_t)n_lambda, pK = (size_t)p * (size_t)K;
  cov_wide_group_path_body<kWidth>(S + set * (size_t)ld * (size_t)p, Sd + set * (size_t)p, ct + set * pK, p, K, ld, alpha + at, beta + at,
                                   n_lambda, ridge_jobs[job], max_iter, tol, W + at * pK, G + at * pK, sweeps_out + at, unconverged + at);
}

// ---- the folds of wide multi-response mode (wmcovariance_cv_run): mcov_assemble_kernel's work, written in the wide layout ----
// mcov_assemble_kernel is one workgroup per training set with the sums s and the shifts d of the p + K columns in dynamic
// LDS and a G x p x (p + K) re-centred matrix for its output; at 3709 features neither belongs there.  As for one response
// (wcov_cv_stats_kernel, wcov_cv_assemble_kernel) the work is cut in two, s and d live in GLOBAL memory, and a column of S_T
// comes straight from row j of the group moments:
//   wmcov_cv_stats_kernel     blockIdx.x = training set T: everything of size p + K or smaller
//   wmcov_cv_assemble_kernel  blockIdx.x = column j, blockIdx.y = T: column j of S_T, diag S_T and row j of c~_T
// WcovSet and wcov_recentred are shared with them: the moments are (p + K + 1) x (p + K + 1) here.

// blockIdx.x = training set T.  mcov_assemble_kernel's expressions for what is per T or per job:
//   s, d   G x (p + K): T's sums of deviations about the common centre and its shifts (every response; a feature only when centred)
//   cst    G x (p + K): the column is constant on T (cov_constant_on_set): scale / divisor 1, zeros in S_T and c~_T
//   scale  G x p      mean  G x (p + K): as mcov_assemble_kernel leaves it      ysd  G x K: the divisors of the responses
//   tstat  3 x G: n_T | y~'y~ | the null deviance, both summed in the order r = 0 .. K - 1
//   l2, l1  jobs x n_lambda, job = mix * G + T      ridge  jobs
// Lane 0 forms yy and the null deviance from the moments themselves: nothing is staged and no barrier is needed.
__global__ __launch_bounds__(kBlock) void wmcov_cv_stats_kernel(const double* __restrict__ Mg, const double* __restrict__ total,
                                                                 const double* __restrict__ mu, int n_groups, int p, int K, int rest,
                                                                 int centre, int standardize, int standardize_response,
                                                                 const double* __restrict__ mix, const double* __restrict__ lambda,
                                                                 int n_mix, int n_lambda, double* __restrict__ s, double* __restrict__ d,
                                                                 int32_t* __restrict__ cst, double* __restrict__ scale, double* __restrict__ mean,
                                                                 double* __restrict__ ysd, double* __restrict__ tstat,
                                                                 double* __restrict__ l2, double* __restrict__ l1,
                                                                 int32_t* __restrict__ ridge) {
  const int t = blockIdx.x, tid = threadIdx.x, nc = p + K, Pa = nc + 1;
  const WcovSet C{Mg + (size_t)t * Pa * Pa, total, Pa, rest};
  const double nT = C(nc, nc);
  const int n_summed = rest ? n_groups : 0;
  // the sd response r is divided by (1 without standardize_response; a response constant on T: 1), from its re-centred square q
  auto sd_y = [&](double q, bool constant) -> double { return (!standardize_response || constant) ? 1.0 : sqrt(q / nT); };
  for (int j = tid; j < nc; j += kBlock) {
    const double sj = C(j, nc), dj = (j >= p || centre) ? sj / nT : 0.0;
    s[(size_t)t * nc + j] = sj;
    d[(size_t)t * nc + j] = dj;
    const double q = wcov_recentred(C(j, j), sj, dj, sj, dj, nT);
    const bool cj = cov_constant_on_set(q, C.magnitude(j, j), C.magnitude(j, nc), dj, nT, n_summed);
    cst[(size_t)t * nc + j] = cj ? 1 : 0;
    if (j < p) {
      scale[(size_t)t * p + j] = (standardize && !cj) ? sqrt(q / nT) : 1.0;
      mean[(size_t)t * nc + j] = centre ? mu[j] + dj : 0.0;
    } else {
      ysd[(size_t)t * K + (j - p)] = sd_y(q, cj);
      mean[(size_t)t * nc + j] = standardize_response ? 0.0 : mu[j + K] + dj;
    }
  }
  if (tid == 0) {
    double yy = 0.0, nulldev = 0.0;
    for (int r = 0; r < K; ++r) {
      const double sr = C(p + r, nc), dr = sr / nT;
      const double qr = wcov_recentred(C(p + r, p + r), sr, dr, sr, dr, nT);
      const bool cr = cov_constant_on_set(qr, C.magnitude(p + r, p + r), C.magnitude(p + r, nc), dr, nT, n_summed);
      const double q = cr ? 0.0 : qr, sd = sd_y(qr, cr);
      nulldev += q;
      yy += q / sd / sd;
    }
    tstat[t] = nT;
    tstat[n_groups + t] = yy;
    tstat[2 * n_groups + t] = nulldev;
  }
  for (int e = tid; e < n_mix * n_lambda; e += kBlock) {
    const int a = e / n_lambda, l = e - a * n_lambda;
    const size_t at = ((size_t)a * n_groups + t) * n_lambda + l;
    l2[at] = (1.0 - mix[a]) * lambda[e];
    l1[at] = mix[a] * lambda[e];
    if (l == 0) ridge[(size_t)a * n_groups + t] = mix[a] == 0.0 ? 1 : 0;
  }
}

// blockIdx.x = column j < p, blockIdx.y = training set T.  Column j of S_T = M^T / n_T / (sd sd') in the layout
// cov_wide_group_path_kernel reads (leading dimension ld, rows p .. ld - 1 the zero pad; set stride ld p), diag S_T and
// c~_T[j, r] = M^T[j, p + r] / sd_y(r) / n_T / sd_j at j K + r (set stride p K): the arithmetic of mcov_assemble_kernel
// followed by cov_wide_group_scale_kernel's.  The moments are read along row j (coalesced; row j is column j bit for bit);
// s, d, scale and the responses' divisors come from wmcov_cv_stats_kernel.
__global__ __launch_bounds__(kBlock) void wmcov_cv_assemble_kernel(const double* __restrict__ Mg, const double* __restrict__ total,
                                                                    const double* __restrict__ s, const double* __restrict__ d,
                                                                    const int32_t* __restrict__ cst, const double* __restrict__ scale,
                                                                    const double* __restrict__ ysd, const double* __restrict__ tstat, int p, int K,
                                                                    int ld, int rest, double* __restrict__ S, double* __restrict__ Sd,
                                                                    double* __restrict__ ct) {
  const int j = blockIdx.x, t = blockIdx.y, nc = p + K, Pa = nc + 1;
  const WcovSet C{Mg + (size_t)t * Pa * Pa, total, Pa, rest};
  s += (size_t)t * nc;
  d += (size_t)t * nc;
  cst += (size_t)t * nc;
  scale += (size_t)t * p;
  ysd += (size_t)t * K;
  const double nT = tstat[t];
  const double sj = s[j], dj = d[j], fj = scale[j];
  const bool cj = cst[j] != 0;
  double* col = S + ((size_t)t * p + j) * (size_t)ld;
  for (int k = threadIdx.x; k < ld; k += kBlock) {
    double v = 0.0;
    if (k < p && !cj && !cst[k]) {
      const double c = C(j, k), sk = s[k], dk = d[k], fk = scale[k];
      v = k >= j ? wcov_recentred(c, sj, dj, sk, dk, nT) / nT / (fj * fk) : wcov_recentred(c, sk, dk, sj, dj, nT) / nT / (fk * fj);
    }
    col[k] = v;
    if (k == j) Sd[(size_t)t * p + j] = v;
  }
  for (int r = threadIdx.x; r < K; r += kBlock)
    ct[((size_t)t * p + j) * K + r] = (cj || cst[p + r]) ? 0.0 : wcov_recentred(C(j, p + r), sj, dj, s[p + r], d[p + r], nT) / ysd[r] / nT / fj;
}

// The wide group kernel's workgroup: both widths give the same bits; profiles/wmcovariance_path.txt has the path kernel's
// time for each (100 lambdas, mix 0.5, default tolerance):
//   lanes    300 x 174, K = 10    4000 x 9, K = 3    2000 x 1000, K = 3    500 x 3000, K = 2
//   256           124 ms              1.3 ms               389 ms               2180 ms
//   1024          181 ms              1.9 ms               413 ms               1476 ms
// Up to 1000 features a column is at most two strides of 256 lanes, and twelve more wavefronts cost more at the barriers
// than they save; at 3000 the sixteen wavefronts win by a third.  So: 256 lanes up to 1024 features, 1024 beyond (not
// wide_cd_width's 512: a move here spends its time on K responses per 16-byte load, not on the load).  No column is
// requested ahead: not measured yet.
constexpr int wmcov_path_width(int p) { return p <= 1024 ? kWideNarrow : kWideFull; }

struct Events {
  hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
  hipStream_t st = nullptr;
  ~Events() {
    for (hipEvent_t v : e)
      if (v) (void)hipEventDestroy(v);
    if (st) (void)hipStreamDestroy(st);
  }
  // the run's own non-blocking stream and the four events its phases are timed between
  hipError_t open() {
    hipError_t err = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    for (hipEvent_t& v : e)
      if (err == hipSuccess) err = hipEventCreate(&v);
    return err;
  }
};

// Diagnostics (covariance.hpp: CovTap): `count` doubles (words) at dev, copied behind whatever the stream holds so far.
// Nothing happens without a tap.  The vectors live in the tap's maps, so they stay where they are until the stream is drained.
hipError_t tap_f64(CovTap* tap, const char* name, const double* dev, size_t count, hipStream_t st) {
  if (!tap) return hipSuccess;
  std::vector<double>& v = tap->f64[name];
  v.resize(count);
  return count ? hipMemcpyAsync(v.data(), dev, sizeof(double) * count, hipMemcpyDeviceToHost, st) : hipSuccess;
}
hipError_t tap_i32(CovTap* tap, const char* name, const int32_t* dev, size_t count, hipStream_t st) {
  if (!tap) return hipSuccess;
  std::vector<int32_t>& v = tap->i32[name];
  v.resize(count);
  return count ? hipMemcpyAsync(v.data(), dev, sizeof(int32_t) * count, hipMemcpyDeviceToHost, st) : hipSuccess;
}
// Behind the path kernel: the four buffers it wrote (coefs = jobs x L x p x K doubles, paths = jobs x L words) and the
// stopping rule it was handed
hipError_t tap_path(CovTap* tap, const double* W, const double* G, size_t coefs, const int32_t* sweeps, const int32_t* unconverged,
                    size_t paths, double tol, unsigned max_iter, hipStream_t st) {
  if (!tap) return hipSuccess;
  tap->f64["tol"].assign(1, tol);
  tap->f64["max_iter"].assign(1, (double)max_iter);
  hipError_t e;
  if ((e = tap_f64(tap, "W", W, coefs, st)) != hipSuccess || (e = tap_f64(tap, "G", G, coefs, st)) != hipSuccess ||
      (e = tap_i32(tap, "sweeps", sweeps, paths, st)) != hipSuccess)
    return e;
  return tap_i32(tap, "unconverged", unconverged, paths, st);
}

// `count` values at offset off of the arena into v, behind whatever the stream holds so far
template <class T>
hipError_t download(const Arena& A, size_t off, size_t count, std::vector<T>* v, hipStream_t st) {
  v->resize(count);
  return count ? hipMemcpyAsync(v->data(), A.base + off, sizeof(T) * count, hipMemcpyDeviceToHost, st) : hipSuccess;
}

static_assert(kTileRows == kMomentTileRows && kTileCols == 16, "group_rows.hpp and wide_layout.hpp count these tiles");

// The moments stage of all six runs: the inputs on the device (x sparse or dense, y as n x K, the parameter vectors of the
// mode), the centres mu, the dense pass's partial tiles and the moment matrices, and the launches from the ones to the others.
//   a fit (G = 0):  one ncols x ncols matrix over ncols = p + K columns, plain row chunks of the n rows;
//   a CV (G > 0):   one per group over ncols = p + K + 1 columns (the last: the ones), and their total; dense x reads its
//                   rows through a GroupRows, sparse x takes a row's group from fold.
// responses: the K response columns of the mcovariance modes (false: the one response of the covariance modes).  The CV form
// alone tells them apart: cov_group_response_kernel against cov_response_centre_kernel + cov_group_responses_kernel, and mu of
// p + 2 against p + 2 K entries (the features' centres | the responses' sums | their means).
struct Moments {
  struct Param {
    size_t off;
    const double* host;
    size_t count;
  };
  const int64_t n;
  const int p, K, G, ncols, pairs, centre;
  const bool sparse, responses;
  const int64_t nnz, rows_per_chunk;     // (rows_per_chunk: what the tile kernel is handed, 0 with a GroupRows)
  const size_t chunks, mu_len, M_elems;
  const AscendingColumns cols;
  const double* const x_dense;
  const int32_t* const colptr;
  const double* const y;
  const int32_t* const fold;
  const GroupRows* const rows;
  std::vector<Param> params;
  size_t o_x = 0, o_colptr = 0, o_rowidx = 0, o_fold = 0, o_perm = 0, o_cbegin = 0, o_gchunk = 0, o_y = 0, o_mu = 0, o_part = 0, o_M = 0, o_total = 0;

  // pb: any of the four problems, validated.  A CV hands over its groups: fold and, for dense x, the rows by group.
  template <class Problem>
  Moments(const Problem& pb, int K_, bool responses_, bool wide, int G_ = 0, const int32_t* fold_ = nullptr, const GroupRows* rows_ = nullptr)
      : n(pb.n), p((int)pb.p), K(K_), G(G_), ncols(p + K + (G ? 1 : 0)), pairs((int)wide_tile_pairs(ncols)), centre(pb.centre ? 1 : 0),
        sparse(pb.x_dense == nullptr), responses(responses_), nnz(sparse ? pb.colptr[p] : 0),
        rows_per_chunk(G ? 0 : cov_rows_per_chunk(n, ncols, wide)),
        chunks(sparse ? 0 : (G ? rows_->chunks() : (size_t)((n + rows_per_chunk - 1) / rows_per_chunk))),
        mu_len((size_t)(G && responses ? p + 2 * K : p + K + 1)), M_elems((size_t)ncols * (size_t)ncols),
        cols(sparse ? pb.colptr : (const int32_t*)nullptr, pb.rowidx, pb.values, sparse ? p : 0), x_dense(pb.x_dense), colptr(pb.colptr),
        y(pb.y), fold(fold_), rows(sparse ? nullptr : rows_) {}

  void reserve(Arena& A) {
    o_x = A.reserve(sizeof(double) * (size_t)(sparse ? nnz : n * (int64_t)p));
    o_colptr = A.reserve(sparse ? sizeof(int32_t) * (size_t)(p + 1) : 0);
    o_rowidx = A.reserve(sparse ? sizeof(int32_t) * (size_t)nnz : 0);
    o_fold = A.reserve(sparse && G ? sizeof(int32_t) * (size_t)n : 0);
    o_perm = A.reserve(rows ? sizeof(int64_t) * (size_t)n : 0);
    o_cbegin = A.reserve(rows ? sizeof(int64_t) * (chunks + 1) : 0);
    o_gchunk = A.reserve(rows ? sizeof(int32_t) * ((size_t)G + 1) : 0);
    o_y = A.reserve(sizeof(double) * (size_t)n * (size_t)K);
    o_mu = A.reserve(sizeof(double) * mu_len);
    o_part = A.reserve(sizeof(double) * chunks * (size_t)pairs * kBlock);
    o_M = A.reserve(sizeof(double) * (size_t)(G ? G : 1) * M_elems);
    o_total = A.reserve(G ? sizeof(double) * M_elems : 0);
  }
  // a parameter vector of the mode (scale, the penalties, the mixes, ...): reserved here, uploaded behind y in this order
  size_t param(Arena& A, const double* host, size_t count) {
    params.push_back({A.reserve(sizeof(double) * count), host, count});
    return params.back().off;
  }

  hipError_t upload(const Arena& A, hipStream_t st) const {
    hipError_t e = hipSuccess;
    auto up = [&](size_t off, const void* src, size_t bytes) {
      if (e == hipSuccess && bytes) e = hipMemcpyAsync(A.base + off, src, bytes, hipMemcpyHostToDevice, st);
    };
    if (sparse) {
      up(o_x, cols.values, sizeof(double) * (size_t)nnz);
      up(o_rowidx, cols.rowidx, sizeof(int32_t) * (size_t)nnz);
      up(o_colptr, colptr, sizeof(int32_t) * (size_t)(p + 1));
      if (G) up(o_fold, fold, sizeof(int32_t) * (size_t)n);
    } else {
      up(o_x, x_dense, sizeof(double) * (size_t)(n * (int64_t)p));
      if (rows) {
        up(o_perm, rows->perm.data(), sizeof(int64_t) * (size_t)n);
        up(o_cbegin, rows->chunk_begin.data(), sizeof(int64_t) * (chunks + 1));
        up(o_gchunk, rows->group_chunk.data(), sizeof(int32_t) * ((size_t)G + 1));
      }
    }
    up(o_y, y, sizeof(double) * (size_t)n * (size_t)K);
    for (const Param& q : params) up(q.off, q.host, sizeof(double) * q.count);
    return e;
  }

  // mu and the moment matrix at o_M.  The caller asks hipGetLastError.
  void launch_fit(const Arena& A, hipStream_t st) const {
    const double* d_x = A.at<double>(o_x);
    const double* d_y = A.at<double>(o_y);
    double* d_mu = A.at<double>(o_mu);
    const int32_t* none = nullptr;
    if (sparse) {
      hipLaunchKernelGGL(cov_sum_kernel<true>, dim3((unsigned)ncols), dim3(kBlock), 0, st, d_x, A.at<int32_t>(o_colptr), d_y, n, p, K, centre, d_mu);
      hipLaunchKernelGGL(cov_sparse_pair_kernel<false>, dim3((unsigned)p, (unsigned)ncols), dim3(kBlock), 0, st, A.at<int32_t>(o_colptr),
                         A.at<int32_t>(o_rowidx), d_x, d_y, d_mu, n, p, K, none, A.at<double>(o_M));
    } else {
      hipLaunchKernelGGL(cov_sum_kernel<false>, dim3((unsigned)ncols), dim3(kBlock), 0, st, d_x, none, d_y, n, p, K, centre, d_mu);
      hipLaunchKernelGGL(cov_dense_tile_kernel, dim3((unsigned)pairs, (unsigned)chunks), dim3(kBlock), 0, st, d_x, d_y, d_mu, n, p, K, ncols,
                         rows_per_chunk, (const int64_t*)nullptr, (const int64_t*)nullptr, A.at<double>(o_part));
      hipLaunchKernelGGL(cov_reduce_kernel, dim3((unsigned)pairs), dim3(kBlock), 0, st, A.at<double>(o_part), (int)chunks, none, ncols,
                         A.at<double>(o_M));
    }
  }
  // the CV form (below, before the CV runs): mu and the groups' matrices at o_M; their total, for a CV that trains on the
  // rest; a CV's taps of what this stage left
  void launch_cv(const Arena& A, hipStream_t st) const;
  void launch_total(const Arena& A, hipStream_t st) const;
  hipError_t tap_cv(const Arena& A, CovTap* tap, bool rest, hipStream_t st) const;
};

// What a path kernel writes over `jobs` jobs of L lambdas and pK coefficients each: W, G, sweeps, unconverged and, where the
// kernel leaves c~ per job (own_c: the narrow kernels and the wide fits' scale kernels), c
struct PathOut {
  const size_t coefs, paths, c_len;
  const bool own_c;
  const size_t o_W, o_G, o_c, o_sweeps, o_unconv;
  PathOut(Arena& A, size_t jobs, int L, size_t pK, bool own_c_)
      : coefs(jobs * (size_t)L * pK), paths(jobs * (size_t)L), c_len(jobs * pK), own_c(own_c_), o_W(A.reserve(sizeof(double) * coefs)),
        o_G(A.reserve(sizeof(double) * coefs)), o_c(A.reserve(own_c ? sizeof(double) * c_len : 0)), o_sweeps(A.reserve(sizeof(int32_t) * paths)),
        o_unconv(A.reserve(sizeof(int32_t) * paths)) {}
  // behind the path kernel: the tap's copies of the four buffers, then the result's (R: any of the four results; c is only
  // sized where it is not the kernel's own)
  template <class R>
  hipError_t fetch(const Arena& A, CovTap* tap, double tol, unsigned max_iter, R* out, hipStream_t st) const {
    // every vector is sized before the first copy: a copy into pageable memory waits for the path kernel, and zero-filling
    // W and G (120 MB each in a wide 50-job CV) belongs in that wait, not behind it
    out->c.resize(c_len);
    out->w.resize(coefs);
    out->g.resize(coefs);
    out->sweeps.resize(paths);
    out->unconverged.resize(paths);
    hipError_t e = tap_path(tap, A.at<double>(o_W), A.at<double>(o_G), coefs, A.at<int32_t>(o_sweeps), A.at<int32_t>(o_unconv), paths, tol, max_iter, st);
    if (e == hipSuccess && own_c) e = download(A, o_c, c_len, &out->c, st);
    if (e == hipSuccess) e = download(A, o_W, coefs, &out->w, st);
    if (e == hipSuccess) e = download(A, o_G, coefs, &out->g, st);
    if (e == hipSuccess) e = download(A, o_sweeps, paths, &out->sweeps, st);
    if (e == hipSuccess) e = download(A, o_unconv, paths, &out->unconverged, st);
    return e;
  }
};

// covariance_run and wcovariance_run: the moments stage and the path outputs around two path kernels.
// wide: S goes to global memory (wide_scale_kernel) and cov_wide_path_kernel<width> runs the path; the dense row
// chunks follow wide_row_chunks.  Not wide: exactly the launches covariance mode has always made.
int cov_run(const CovarianceProblem& pb, CovarianceResult* out, bool wide, int width, CovTap* tap) {
  const int64_t n = pb.n;
  const int p = (int)pb.p, P1 = p + 1, L = pb.n_lambda;
  const bool sparse = pb.x_dense == nullptr;
  if (n <= 0 || p <= 0 || pb.p > (wide ? kWcovMaxFeatures : kCovMaxFeatures) || L <= 0 || (wide && width != kWideNarrow && width != kWideFull) ||
      (!sparse && pb.colptr) || (sparse && (!pb.colptr || !pb.rowidx || !pb.values))) {
    set_error("%s: invalid problem", wide ? "wcovariance_run" : "covariance_run");
    return SGDNET_EINVAL;
  }
  SGD_HIP_TRY(hipSetDevice(pb.device));

  Arena A;
  Moments m(pb, 1, false, wide);
  m.reserve(A);
  const size_t o_scale = m.param(A, pb.scale, (size_t)p), o_alpha = m.param(A, pb.alpha, (size_t)L), o_beta = m.param(A, pb.beta, (size_t)L);
  const int ld = (int)wide_leading_dim(p);
  const size_t o_S = A.reserve(wide ? sizeof(double) * (size_t)ld * (size_t)p : 0);
  const size_t o_Sd = A.reserve(wide ? sizeof(double) * (size_t)p : 0);
  const PathOut po(A, 1, L, (size_t)p, true);
  SGD_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&A.base), A.used));

  Events ev;
  SGD_HIP_TRY(ev.open());
  hipStream_t st = ev.st;
  double* d_M = A.at<double>(m.o_M);
  SGD_HIP_TRY(m.upload(A, st));
  SGD_HIP_TRY(hipEventRecord(ev.e[0], st));
  m.launch_fit(A, st);
  SGD_HIP_TRY(hipGetLastError());
  SGD_HIP_TRY(hipEventRecord(ev.e[1], st));
  SGD_HIP_TRY(tap_f64(tap, "mu", A.at<double>(m.o_mu), (size_t)P1 + 1, st));     // (the last entry: mean of y)
  SGD_HIP_TRY(tap_f64(tap, "M", d_M, (size_t)P1 * (size_t)P1, st));
  if (wide) {
    hipLaunchKernelGGL(wide_scale_kernel, dim3((unsigned)p), dim3(kBlock), 0, st, d_M, A.at<double>(o_scale), p, P1, ld, (double)n,
                       A.at<double>(o_S), A.at<double>(o_Sd), A.at<double>(po.o_c));
    SGD_HIP_TRY(hipGetLastError());
    SGD_HIP_TRY(hipEventRecord(ev.e[3], st));
    SGD_HIP_TRY(tap_f64(tap, "S", A.at<double>(o_S), (size_t)ld * (size_t)p, st));
    SGD_HIP_TRY(tap_f64(tap, "Sd", A.at<double>(o_Sd), (size_t)p, st));
    SGD_HIP_TRY(tap_f64(tap, "ct", A.at<double>(po.o_c), (size_t)p, st));
    static const int ahead = exp_env_int("SGDNET_WCOV_PREFETCH", -1);     // (0 / 1: profiles/wcovariance_path.txt)
    const bool prefetch = ahead < 0 ? wcov_path_ahead(p) : ahead != 0;
    const auto kernel = width == kWideNarrow ? (prefetch ? cov_wide_path_kernel<kWideNarrow, true> : cov_wide_path_kernel<kWideNarrow, false>)
                                             : (prefetch ? cov_wide_path_kernel<kWideFull, true> : cov_wide_path_kernel<kWideFull, false>);
    hipLaunchKernelGGL(kernel, dim3(1), dim3((unsigned)width), 0, st, A.at<double>(o_S), A.at<double>(o_Sd), A.at<double>(po.o_c), p, ld,
                       A.at<double>(o_alpha), A.at<double>(o_beta), L, pb.ridge ? 1 : 0, pb.max_iter, pb.tol, A.at<double>(po.o_W),
                       A.at<double>(po.o_G), A.at<int32_t>(po.o_sweeps), A.at<int32_t>(po.o_unconv));
  } else {
    hipLaunchKernelGGL(cov_path_kernel, dim3(1), dim3(64), 0, st, d_M, A.at<double>(o_scale), p, 1, (double)n, (const double*)nullptr,
                       A.at<double>(o_alpha), A.at<double>(o_beta), L, pb.ridge ? 1 : 0, (const int32_t*)nullptr, pb.max_iter, pb.tol,
                       A.at<double>(po.o_W), A.at<double>(po.o_G), A.at<double>(po.o_c), A.at<int32_t>(po.o_sweeps), A.at<int32_t>(po.o_unconv));
  }
  SGD_HIP_TRY(hipGetLastError());
  SGD_HIP_TRY(hipEventRecord(ev.e[2], st));
  SGD_HIP_TRY(po.fetch(A, tap, pb.tol, pb.max_iter, out, st));
  SGD_HIP_TRY(download(A, m.o_mu, (size_t)p, &out->mean, st));
  SGD_HIP_TRY(hipStreamSynchronize(st));
  SGD_HIP_TRY(hipEventElapsedTime(&out->moments_ms, ev.e[0], ev.e[1]));
  if (wide) {
    SGD_HIP_TRY(hipEventElapsedTime(&out->scale_ms, ev.e[1], ev.e[3]));
    SGD_HIP_TRY(hipEventElapsedTime(&out->path_ms, ev.e[3], ev.e[2]));
  } else {
    SGD_HIP_TRY(hipEventElapsedTime(&out->path_ms, ev.e[1], ev.e[2]));
  }
  return SGDNET_OK;
}

// mcovariance_run and wmcovariance_run: the same stages around two path kernels.
// wide: S and c~ go to global memory (cov_wide_group_scale_kernel) and cov_wide_group_path_kernel<width> runs the path; the
// dense row chunks follow wide_row_chunks.  Not wide: exactly the launches mcovariance mode has always made.
int mcov_run(const McovarianceProblem& pb, McovarianceResult* out, bool wide, int width, CovTap* tap) {
  const int64_t n = pb.n;
  const int p = (int)pb.p, K = pb.K, nc = p + K, L = pb.n_lambda;
  const bool sparse = pb.x_dense == nullptr;
  const bool width_ok = wide ? (width == kWideNarrow || width == kWideFull) : (width == 0 || width == kMcovNarrow || width == kMcovWide);
  if (n <= 0 || p <= 0 || K < 1 || pb.p > (wide ? wmcov_max_features(K) : mcov_max_features(K)) || L <= 0 || !pb.y || !width_ok ||
      (!sparse && pb.colptr) || (sparse && (!pb.colptr || !pb.rowidx || !pb.values))) {
    set_error("%s: invalid problem", wide ? "wmcovariance_run" : "mcovariance_run");
    return SGDNET_EINVAL;
  }
  SGD_HIP_TRY(hipSetDevice(pb.device));
  const size_t pK = (size_t)p * (size_t)K;
  if (width == 0) width = mcov_path_width(pK);

  Arena A;
  Moments m(pb, K, true, wide);
  m.reserve(A);
  const size_t o_scale = m.param(A, pb.scale, (size_t)p), o_alpha = m.param(A, pb.alpha, (size_t)L), o_beta = m.param(A, pb.beta, (size_t)L);
  const int ld = (int)wide_leading_dim(p);
  const size_t o_S = A.reserve(wide ? sizeof(double) * (size_t)ld * (size_t)p : 0);
  const size_t o_Sd = A.reserve(wide ? sizeof(double) * (size_t)p : 0);
  const PathOut po(A, 1, L, pK, true);
  SGD_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&A.base), A.used));

  Events ev;
  SGD_HIP_TRY(ev.open());
  hipStream_t st = ev.st;
  double* d_M = A.at<double>(m.o_M);
  SGD_HIP_TRY(m.upload(A, st));
  SGD_HIP_TRY(hipEventRecord(ev.e[0], st));
  m.launch_fit(A, st);
  SGD_HIP_TRY(hipGetLastError());
  SGD_HIP_TRY(hipEventRecord(ev.e[1], st));
  SGD_HIP_TRY(tap_f64(tap, "mu", A.at<double>(m.o_mu), (size_t)nc, st));
  SGD_HIP_TRY(tap_f64(tap, "M", d_M, (size_t)nc * (size_t)nc, st));
  if (wide) {
    hipLaunchKernelGGL(cov_wide_group_scale_kernel, dim3((unsigned)p), dim3(kBlock), 0, st, d_M, A.at<double>(o_scale), p, K, ld, (double)n,
                       A.at<double>(o_S), A.at<double>(o_Sd), A.at<double>(po.o_c));
    SGD_HIP_TRY(hipGetLastError());
    SGD_HIP_TRY(hipEventRecord(ev.e[3], st));
    SGD_HIP_TRY(tap_f64(tap, "S", A.at<double>(o_S), (size_t)ld * (size_t)p, st));
    SGD_HIP_TRY(tap_f64(tap, "Sd", A.at<double>(o_Sd), (size_t)p, st));
    SGD_HIP_TRY(tap_f64(tap, "ct", A.at<double>(po.o_c), pK, st));
    const auto kernel = width == kWideNarrow ? cov_wide_group_path_kernel<kWideNarrow> : cov_wide_group_path_kernel<kWideFull>;
    hipLaunchKernelGGL(kernel, dim3(1), dim3((unsigned)width), 0, st, A.at<double>(o_S), A.at<double>(o_Sd), A.at<double>(po.o_c), p, K, ld,
                       A.at<double>(o_alpha), A.at<double>(o_beta), L, pb.ridge ? 1 : 0, pb.max_iter, pb.tol, A.at<double>(po.o_W),
                       A.at<double>(po.o_G), A.at<int32_t>(po.o_sweeps), A.at<int32_t>(po.o_unconv));
  } else {
    const auto kernel = width == kMcovNarrow ? cov_group_path_kernel<kMcovNarrow> : cov_group_path_kernel<kMcovWide>;
    hipLaunchKernelGGL(kernel, dim3(1), dim3((unsigned)width), 0, st, d_M, A.at<double>(o_scale), p, K, 1, (double)n, (const double*)nullptr,
                       A.at<double>(o_alpha), A.at<double>(o_beta), L, pb.ridge ? 1 : 0, (const int32_t*)nullptr, pb.max_iter, pb.tol,
                       A.at<double>(po.o_W), A.at<double>(po.o_G), A.at<double>(po.o_c), A.at<int32_t>(po.o_sweeps), A.at<int32_t>(po.o_unconv));
  }
  SGD_HIP_TRY(hipGetLastError());
  SGD_HIP_TRY(hipEventRecord(ev.e[2], st));
  SGD_HIP_TRY(po.fetch(A, tap, pb.tol, pb.max_iter, out, st));
  SGD_HIP_TRY(download(A, m.o_mu, (size_t)p, &out->mean, st));
  SGD_HIP_TRY(hipStreamSynchronize(st));
  SGD_HIP_TRY(hipEventElapsedTime(&out->moments_ms, ev.e[0], ev.e[1]));
  if (wide) {
    SGD_HIP_TRY(hipEventElapsedTime(&out->scale_ms, ev.e[1], ev.e[3]));
    SGD_HIP_TRY(hipEventElapsedTime(&out->path_ms, ev.e[3], ev.e[2]));
  } else {
    SGD_HIP_TRY(hipEventElapsedTime(&out->path_ms, ev.e[1], ev.e[2]));
  }
  return SGDNET_OK;
}

}  // namespace

int covariance_run(const CovarianceProblem& pb, CovarianceResult* out, CovTap* tap) { return cov_run(pb, out, false, 0, tap); }

int wcovariance_run(const CovarianceProblem& pb, CovarianceResult* out, int width, CovTap* tap) {
  return cov_run(pb, out, true, width != 0 ? width : wide_cd_width((int)std::min<int64_t>(pb.p, kWcovMaxFeatures)), tap);
}

int mcovariance_run(const McovarianceProblem& pb, McovarianceResult* out, int width, CovTap* tap) { return mcov_run(pb, out, false, width, tap); }

int wmcovariance_run(const McovarianceProblem& pb, McovarianceResult* out, int width, CovTap* tap) {
  return mcov_run(pb, out, true, width != 0 ? width : wmcov_path_width((int)std::min<int64_t>(pb.p, kWcovMaxFeatures)), tap);
}

// ---- cross-validation: the CV form of the moments stage and what the four CV runs share besides ----
namespace {

void Moments::launch_cv(const Arena& A, hipStream_t st) const {
  const double* d_x = A.at<double>(o_x);
  const double* d_y = A.at<double>(o_y);
  double* d_mu = A.at<double>(o_mu);
  double* d_Mg = A.at<double>(o_M);
  const int32_t* d_colptr = sparse ? A.at<int32_t>(o_colptr) : nullptr;
  const int32_t* d_fold = A.at<int32_t>(o_fold);
  if (sparse) hipLaunchKernelGGL(cov_sum_kernel<true>, dim3((unsigned)(p + K)), dim3(kBlock), 0, st, d_x, d_colptr, d_y, n, p, K, centre, d_mu);
  else hipLaunchKernelGGL(cov_sum_kernel<false>, dim3((unsigned)(p + K)), dim3(kBlock), 0, st, d_x, d_colptr, d_y, n, p, K, centre, d_mu);
  if (responses) hipLaunchKernelGGL(cov_response_centre_kernel, dim3(1), dim3(kBlock), 0, st, d_mu, n, p, K);
  if (sparse) {
    if (responses)
      hipLaunchKernelGGL(cov_group_responses_kernel, dim3((unsigned)K, (unsigned)K, (unsigned)G), dim3(kBlock), 0, st, d_y, d_fold, d_mu, n, p, K,
                         d_Mg);
    else hipLaunchKernelGGL(cov_group_response_kernel, dim3((unsigned)G), dim3(kBlock), 0, st, d_y, d_fold, d_mu, n, p, d_Mg);
    hipLaunchKernelGGL(cov_sparse_pair_kernel<true>, dim3((unsigned)p, (unsigned)ncols, (unsigned)G), dim3(kBlock), 0, st, d_colptr,
                       A.at<int32_t>(o_rowidx), d_x, d_y, d_mu, n, p, K, d_fold, d_Mg);
  } else {
    hipLaunchKernelGGL(cov_dense_tile_kernel, dim3((unsigned)pairs, (unsigned)chunks), dim3(kBlock), 0, st, d_x, d_y, d_mu, n, p, K, ncols,
                       rows_per_chunk, A.at<int64_t>(o_perm), A.at<int64_t>(o_cbegin), A.at<double>(o_part));
    hipLaunchKernelGGL(cov_reduce_kernel, dim3((unsigned)pairs, (unsigned)G), dim3(kBlock), 0, st, A.at<double>(o_part), (int)chunks,
                       A.at<int32_t>(o_gchunk), ncols, d_Mg);
  }
}
// the groups' matrices added in group order
void Moments::launch_total(const Arena& A, hipStream_t st) const {
  hipLaunchKernelGGL(cov_total_kernel, dim3((unsigned)((M_elems + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, A.at<double>(o_M), G, (int)M_elems,
                     A.at<double>(o_total));
}
hipError_t Moments::tap_cv(const Arena& A, CovTap* tap, bool rest, hipStream_t st) const {
  hipError_t e = tap_f64(tap, "mu", A.at<double>(o_mu), mu_len, st);
  if (e == hipSuccess) e = tap_f64(tap, "Mg", A.at<double>(o_M), (size_t)G * M_elems, st);
  if (e == hipSuccess && rest) e = tap_f64(tap, "total", A.at<double>(o_total), M_elems, st);
  return e;
}

// What every CV assembly leaves besides its matrices: per training set scale (p), mean (nc = p + K) and tstat (three
// vectors over the sets); per job the two penalties per lambda and the ridge flag
struct CvSets {
  const size_t G, jobs, scales, means, pens;
  const size_t o_scale, o_mean, o_tstat, o_pen_a, o_pen_b, o_ridge;
  CvSets(Arena& A, int G_, int n_mix, int L, int p, int nc)
      : G((size_t)G_), jobs((size_t)n_mix * G), scales(G * (size_t)p), means(G * (size_t)nc), pens(jobs * (size_t)L),
        o_scale(A.reserve(sizeof(double) * scales)), o_mean(A.reserve(sizeof(double) * means)), o_tstat(A.reserve(sizeof(double) * 3 * G)),
        o_pen_a(A.reserve(sizeof(double) * pens)), o_pen_b(A.reserve(sizeof(double) * pens)), o_ridge(A.reserve(sizeof(int32_t) * jobs)) {}
  hipError_t tap(const Arena& A, CovTap* tap, hipStream_t st) const {
    hipError_t e = tap_f64(tap, "scale", A.at<double>(o_scale), scales, st);
    if (e == hipSuccess) e = tap_f64(tap, "mean", A.at<double>(o_mean), means, st);
    if (e == hipSuccess) e = tap_f64(tap, "tstat", A.at<double>(o_tstat), 3 * G, st);
    if (e == hipSuccess) e = tap_f64(tap, "pen_a", A.at<double>(o_pen_a), pens, st);
    if (e == hipSuccess) e = tap_f64(tap, "pen_b", A.at<double>(o_pen_b), pens, st);
    if (e == hipSuccess) e = tap_i32(tap, "ridge", A.at<int32_t>(o_ridge), jobs, st);
    return e;
  }
  template <class R>
  hipError_t fetch(const Arena& A, R* out, std::vector<double>* tstat, hipStream_t st) const {
    hipError_t e = download(A, o_tstat, 3 * G, tstat, st);
    if (e == hipSuccess) e = download(A, o_mean, means, &out->mean, st);
    if (e == hipSuccess) e = download(A, o_scale, scales, &out->scale, st);
    return e;
  }
  // once the stream is drained: tstat's three vectors
  void split(const std::vector<double>& tstat, std::vector<double>* a, std::vector<double>* b, std::vector<double>* c) const {
    a->assign(tstat.begin(), tstat.begin() + G);
    b->assign(tstat.begin() + G, tstat.begin() + 2 * G);
    c->assign(tstat.begin() + 2 * G, tstat.end());
  }
};

// the wide CV runs: c~ is the training set's (ct: G x len), every mix of a set gets its copy (c: jobs x len, job = mix G + T)
void copy_to_jobs(const std::vector<double>& ct, size_t G, size_t len, std::vector<double>* c) {
  for (size_t job = 0; job * len < c->size(); ++job) std::copy(ct.begin() + (job % G) * len, ct.begin() + (job % G + 1) * len, c->begin() + job * len);
}

// dense x of a CV: the rows by group, in chunks of the size one fit of n rows over ncols columns would use (the summation
// order is a function of (n, ncols, fold) alone).  More than kCovMaxRowChunks chunks are refused by the mode's name.
int cv_group_rows(const char* mode, const int32_t* fold, int64_t n, int G, int ncols, bool wide, GroupRows* rows) {
  if (group_rows(fold, n, G, cov_rows_per_chunk(n, ncols, wide), kCovMaxRowChunks, rows)) return SGDNET_OK;
  set_error("mode = %s needs the rows of the groups in at most %d chunks: %d groups of %lld rows", mode, kCovMaxRowChunks, G, (long long)n);
  return SGDNET_EUNSUPPORTED;
}

}  // namespace

int covariance_cv_run(const CovarianceCvProblem& pb, CovarianceCvResult* out, CovTap* tap) {
  const int64_t n = pb.n;
  const int p = (int)pb.p, P1 = p + 1, Pa = p + 2, L = pb.n_lambda, G = pb.n_groups, A_mix = pb.n_mix;
  const bool sparse = pb.x_dense == nullptr;
  if (n <= 0 || p <= 0 || p > kCovMaxFeatures || L <= 0 || G <= 0 || A_mix <= 0 || !pb.fold || !pb.y || !pb.mix || !pb.lambda ||
      (pb.train_on_rest && G < 2) || (size_t)G * Pa * Pa * sizeof(double) > kCovGroupMomentBytes ||
      (!sparse && pb.colptr) || (sparse && (!pb.colptr || !pb.rowidx || !pb.values))) {
    set_error("covariance_cv_run: invalid problem");
    return SGDNET_EINVAL;
  }
  SGD_HIP_TRY(hipSetDevice(pb.device));
  GroupRows rows;
  if (!sparse)
    if (const int rc = cv_group_rows("covariance", pb.fold, n, G, Pa, false, &rows)) return rc;
  if (sparse && G > kCovMaxRowChunks) {       // (the pair kernel's gridDim.z)
    set_error("mode = covariance needs at most %d groups of sparse rows: %d groups", kCovMaxRowChunks, G);
    return SGDNET_EUNSUPPORTED;
  }
  const int rest = pb.train_on_rest ? 1 : 0;

  Arena A;
  Moments m(pb, 1, false, false, G, pb.fold, &rows);
  m.reserve(A);
  const size_t o_mix = m.param(A, pb.mix, (size_t)A_mix), o_lambda = m.param(A, pb.lambda, (size_t)A_mix * (size_t)L);
  const size_t o_Mt = A.reserve(sizeof(double) * (size_t)G * (size_t)P1 * (size_t)P1);
  const CvSets sets(A, G, A_mix, L, p, P1);
  const PathOut po(A, sets.jobs, L, (size_t)p, true);
  SGD_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&A.base), A.used));

  Events ev;
  SGD_HIP_TRY(ev.open());
  hipStream_t st = ev.st;
  double* d_tstat = A.at<double>(sets.o_tstat);
  SGD_HIP_TRY(m.upload(A, st));
  SGD_HIP_TRY(hipEventRecord(ev.e[0], st));
  m.launch_cv(A, st);
  SGD_HIP_TRY(hipGetLastError());
  SGD_HIP_TRY(hipEventRecord(ev.e[1], st));
  if (rest) m.launch_total(A, st);
  hipLaunchKernelGGL(cov_assemble_kernel, dim3((unsigned)G), dim3(kBlock), 0, st, A.at<double>(m.o_M), A.at<double>(m.o_total),
                     A.at<double>(m.o_mu), G, p, rest, pb.centre ? 1 : 0, pb.standardize ? 1 : 0, A.at<double>(o_mix), A.at<double>(o_lambda),
                     A_mix, L, A.at<double>(o_Mt), A.at<double>(sets.o_scale), A.at<double>(sets.o_mean), d_tstat, A.at<double>(sets.o_pen_a),
                     A.at<double>(sets.o_pen_b), A.at<int32_t>(sets.o_ridge));
  SGD_HIP_TRY(hipGetLastError());
  SGD_HIP_TRY(hipEventRecord(ev.e[2], st));
  if (tap) {
    SGD_HIP_TRY(m.tap_cv(A, tap, pb.train_on_rest, st));
    SGD_HIP_TRY(tap_f64(tap, "Mt", A.at<double>(o_Mt), (size_t)G * (size_t)P1 * (size_t)P1, st));
    SGD_HIP_TRY(sets.tap(A, tap, st));
  }
  hipLaunchKernelGGL(cov_path_kernel, dim3((unsigned)sets.jobs), dim3(64), 0, st, A.at<double>(o_Mt), A.at<double>(sets.o_scale), p, G, 0.0,
                     d_tstat, A.at<double>(sets.o_pen_a), A.at<double>(sets.o_pen_b), L, 0, A.at<int32_t>(sets.o_ridge), pb.max_iter, pb.tol,
                     A.at<double>(po.o_W), A.at<double>(po.o_G), A.at<double>(po.o_c), A.at<int32_t>(po.o_sweeps), A.at<int32_t>(po.o_unconv));
  SGD_HIP_TRY(hipGetLastError());
  SGD_HIP_TRY(hipEventRecord(ev.e[3], st));
  std::vector<double> tstat;
  SGD_HIP_TRY(po.fetch(A, tap, pb.tol, pb.max_iter, out, st));
  SGD_HIP_TRY(sets.fetch(A, out, &tstat, st));
  SGD_HIP_TRY(hipStreamSynchronize(st));
  sets.split(tstat, &out->n_train, &out->y_scale, &out->yy);
  SGD_HIP_TRY(hipEventElapsedTime(&out->moments_ms, ev.e[0], ev.e[1]));
  SGD_HIP_TRY(hipEventElapsedTime(&out->assemble_ms, ev.e[1], ev.e[2]));
  SGD_HIP_TRY(hipEventElapsedTime(&out->path_ms, ev.e[2], ev.e[3]));
  return SGDNET_OK;
}

// covariance_cv_run beyond kCovMaxFeatures features: the same group moments pass (the wide mode's row chunks),
// wcov_cv_stats_kernel and wcov_cv_assemble_kernel instead of cov_assemble_kernel, cov_wide_cv_path_kernel over the jobs.
int wcovariance_cv_run(const CovarianceCvProblem& pb, CovarianceCvResult* out, int width, CovTap* tap) {
  const int64_t n = pb.n;
  const int p = (int)pb.p, P1 = p + 1, Pa = p + 2, L = pb.n_lambda, G = pb.n_groups, A_mix = pb.n_mix;
  const bool sparse = pb.x_dense == nullptr;
  if (n <= 0 || p <= 0 || pb.p > kWcovMaxFeatures || L <= 0 || G <= 0 || A_mix <= 0 || !pb.fold || !pb.y || !pb.mix || !pb.lambda ||
      (pb.train_on_rest && G < 2) || (!sparse && pb.colptr) || (sparse && (!pb.colptr || !pb.rowidx || !pb.values))) {
    set_error("wcovariance_cv_run: invalid problem");
    return SGDNET_EINVAL;
  }
  if (width == 0) width = wide_cd_width(p);
  if (width != kWideNarrow && width != kWideFull) {
    set_error("wcovariance_cv_run: the path kernel's workgroup is %d or %d lanes, not %d", kWideNarrow, kWideFull, width);
    return SGDNET_EINVAL;
  }
  GroupRows rows;
  if (!sparse)
    if (const int rc = cv_group_rows("wcovariance", pb.fold, n, G, Pa, true, &rows)) return rc;
  if (sparse && G > kCovMaxRowChunks) {       // (the pair kernel's gridDim.z, the assembly's gridDim.y)
    set_error("mode = wcovariance needs at most %d groups of sparse rows: %d groups", kCovMaxRowChunks, G);
    return SGDNET_EUNSUPPORTED;
  }
  if (wcov_cv_bytes(G, p, (int64_t)rows.chunks()) > kWcovCvBytes) {
    set_error("mode = wcovariance needs the moments and the scaled matrices of the groups within %zu bytes: %d groups of %d features are %zu bytes",
              kWcovCvBytes, G, p, wcov_cv_bytes(G, p, (int64_t)rows.chunks()));
    return SGDNET_EUNSUPPORTED;
  }
  SGD_HIP_TRY(hipSetDevice(pb.device));
  const int ld = (int)wide_leading_dim(p), rest = pb.train_on_rest ? 1 : 0;

  Arena A;
  Moments m(pb, 1, false, true, G, pb.fold, &rows);      // (Pa^2 is at most 4533^2 = 20 548 089: cov_total_kernel's int)
  m.reserve(A);
  const size_t o_mix = m.param(A, pb.mix, (size_t)A_mix), o_lambda = m.param(A, pb.lambda, (size_t)A_mix * (size_t)L);
  const size_t o_s = A.reserve(sizeof(double) * (size_t)G * (size_t)P1);
  const size_t o_d = A.reserve(sizeof(double) * (size_t)G * (size_t)P1);
  const size_t o_cst = A.reserve(sizeof(int32_t) * (size_t)G * (size_t)P1);
  const size_t o_S = A.reserve(sizeof(double) * (size_t)G * (size_t)ld * (size_t)p);
  const size_t o_Sd = A.reserve(sizeof(double) * (size_t)G * (size_t)p);
  const size_t o_ct = A.reserve(sizeof(double) * (size_t)G * (size_t)p);
  const CvSets sets(A, G, A_mix, L, p, P1);
  const PathOut po(A, sets.jobs, L, (size_t)p, false);
  SGD_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&A.base), A.used));

  Events ev;
  SGD_HIP_TRY(ev.open());
  hipStream_t st = ev.st;
  double* d_Mg = A.at<double>(m.o_M);
  double* d_total = A.at<double>(m.o_total);
  double* d_tstat = A.at<double>(sets.o_tstat);
  SGD_HIP_TRY(m.upload(A, st));
  SGD_HIP_TRY(hipEventRecord(ev.e[0], st));
  m.launch_cv(A, st);
  if (rest) m.launch_total(A, st);
  SGD_HIP_TRY(hipGetLastError());
  SGD_HIP_TRY(hipEventRecord(ev.e[1], st));
  hipLaunchKernelGGL(wcov_cv_stats_kernel, dim3((unsigned)G), dim3(kBlock), 0, st, d_Mg, d_total, A.at<double>(m.o_mu), G, p, rest,
                     pb.centre ? 1 : 0, pb.standardize ? 1 : 0, A.at<double>(o_mix), A.at<double>(o_lambda), A_mix, L, A.at<double>(o_s),
                     A.at<double>(o_d), A.at<int32_t>(o_cst), A.at<double>(sets.o_scale), A.at<double>(sets.o_mean), d_tstat,
                     A.at<double>(sets.o_pen_a), A.at<double>(sets.o_pen_b), A.at<int32_t>(sets.o_ridge));
  hipLaunchKernelGGL(wcov_cv_assemble_kernel, dim3((unsigned)p, (unsigned)G), dim3(kBlock), 0, st, d_Mg, d_total, A.at<double>(o_s),
                     A.at<double>(o_d), A.at<int32_t>(o_cst), A.at<double>(sets.o_scale), d_tstat, G, p, ld, rest, A.at<double>(o_S),
                     A.at<double>(o_Sd), A.at<double>(o_ct));
  SGD_HIP_TRY(hipGetLastError());
  SGD_HIP_TRY(hipEventRecord(ev.e[2], st));
  if (tap) {
    SGD_HIP_TRY(m.tap_cv(A, tap, pb.train_on_rest, st));
    SGD_HIP_TRY(tap_f64(tap, "s", A.at<double>(o_s), (size_t)G * (size_t)P1, st));
    SGD_HIP_TRY(tap_f64(tap, "d", A.at<double>(o_d), (size_t)G * (size_t)P1, st));
    SGD_HIP_TRY(sets.tap(A, tap, st));
    SGD_HIP_TRY(tap_f64(tap, "S", A.at<double>(o_S), (size_t)G * (size_t)ld * (size_t)p, st));
    SGD_HIP_TRY(tap_f64(tap, "Sd", A.at<double>(o_Sd), (size_t)G * (size_t)p, st));
    SGD_HIP_TRY(tap_f64(tap, "ct", A.at<double>(o_ct), (size_t)G * (size_t)p, st));
  }
  static const int ahead = exp_env_int("SGDNET_WCOV_PREFETCH", -1);     // (0 / 1, as in wcovariance_run)
  const bool prefetch = ahead < 0 ? wcov_path_ahead(p) : ahead != 0;
  const auto kernel = width == kWideNarrow ? (prefetch ? cov_wide_cv_path_kernel<kWideNarrow, true> : cov_wide_cv_path_kernel<kWideNarrow, false>)
                                           : (prefetch ? cov_wide_cv_path_kernel<kWideFull, true> : cov_wide_cv_path_kernel<kWideFull, false>);
  hipLaunchKernelGGL(kernel, dim3((unsigned)sets.jobs), dim3((unsigned)width), 0, st, A.at<double>(o_S), A.at<double>(o_Sd), A.at<double>(o_ct), p,
                     ld, G, A.at<double>(sets.o_pen_a), A.at<double>(sets.o_pen_b), L, A.at<int32_t>(sets.o_ridge), pb.max_iter, pb.tol,
                     A.at<double>(po.o_W), A.at<double>(po.o_G), A.at<int32_t>(po.o_sweeps), A.at<int32_t>(po.o_unconv));
  SGD_HIP_TRY(hipGetLastError());
  SGD_HIP_TRY(hipEventRecord(ev.e[3], st));
  std::vector<double> tstat, ct;
  SGD_HIP_TRY(po.fetch(A, tap, pb.tol, pb.max_iter, out, st));
  SGD_HIP_TRY(sets.fetch(A, out, &tstat, st));
  SGD_HIP_TRY(download(A, o_ct, (size_t)G * (size_t)p, &ct, st));
  SGD_HIP_TRY(hipStreamSynchronize(st));
  copy_to_jobs(ct, (size_t)G, (size_t)p, &out->c);
  sets.split(tstat, &out->n_train, &out->y_scale, &out->yy);
  SGD_HIP_TRY(hipEventElapsedTime(&out->moments_ms, ev.e[0], ev.e[1]));
  SGD_HIP_TRY(hipEventElapsedTime(&out->assemble_ms, ev.e[1], ev.e[2]));
  SGD_HIP_TRY(hipEventElapsedTime(&out->path_ms, ev.e[2], ev.e[3]));
  return SGDNET_OK;
}

// covariance_cv_run for K responses: the same group moments with the columns p .. p + K - 1 the responses and column p + K the
// ones, mcov_assemble_kernel, and cov_group_path_kernel over the jobs.
int mcovariance_cv_run(const McovarianceCvProblem& pb, McovarianceCvResult* out, CovTap* tap) {
  const int64_t n = pb.n;
  const int p = (int)pb.p, K = pb.K, nc = p + K, Pa = nc + 1, L = pb.n_lambda, G = pb.n_groups, A_mix = pb.n_mix;
  const bool sparse = pb.x_dense == nullptr;
  const bool width_ok = pb.width == 0 || pb.width == kMcovNarrow || pb.width == kMcovWide;
  if (n <= 0 || p <= 0 || K < 1 || pb.p > mcov_max_features(K) || L <= 0 || G <= 0 || A_mix <= 0 || !pb.fold || !pb.y || !pb.mix ||
      !pb.lambda || !width_ok || (pb.train_on_rest && G < 2) || mcov_group_moment_bytes(G, p, K) > kCovGroupMomentBytes ||
      (!sparse && pb.colptr) || (sparse && (!pb.colptr || !pb.rowidx || !pb.values))) {
    set_error("mcovariance_cv_run: invalid problem");
    return SGDNET_EINVAL;
  }
  const size_t pK = (size_t)p * (size_t)K;
  const int width = pb.width != 0 ? pb.width : mcov_path_width(pK);
  // dense x: the rows by group as covariance_cv_run cuts them (gridDim.y of the tile kernel); sparse x: gridDim.z of the pair kernel
  GroupRows rows;
  if (sparse ? G > kCovMaxRowChunks : !group_rows(pb.fold, n, G, cov_rows_per_chunk(n, Pa, false), kCovMaxRowChunks, &rows)) {
    set_error("mcovariance_cv_run: more than %d row chunks or groups", kCovMaxRowChunks);
    return SGDNET_EINVAL;
  }
  SGD_HIP_TRY(hipSetDevice(pb.device));
  const int rest = pb.train_on_rest ? 1 : 0;

  Arena A;
  Moments m(pb, K, true, false, G, pb.fold, &rows);
  m.reserve(A);
  const size_t o_mix = m.param(A, pb.mix, (size_t)A_mix), o_lambda = m.param(A, pb.lambda, (size_t)A_mix * (size_t)L);
  const size_t o_Mt = A.reserve(sizeof(double) * (size_t)G * (size_t)p * (size_t)nc);
  const CvSets sets(A, G, A_mix, L, p, nc);      // (pen_a: the l2 strengths, pen_b: the group thresholds)
  const PathOut po(A, sets.jobs, L, pK, true);
  SGD_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&A.base), A.used));

  Events ev;
  SGD_HIP_TRY(ev.open());
  hipStream_t st = ev.st;
  double* d_tstat = A.at<double>(sets.o_tstat);
  SGD_HIP_TRY(m.upload(A, st));
  SGD_HIP_TRY(hipEventRecord(ev.e[0], st));
  m.launch_cv(A, st);
  SGD_HIP_TRY(hipGetLastError());
  SGD_HIP_TRY(hipEventRecord(ev.e[1], st));
  if (rest) m.launch_total(A, st);
  // (20 (p + K) bytes of LDS: the moment budget keeps p + K + 1 below 2897, so below 57 920 bytes of the 64 KiB)
  hipLaunchKernelGGL(mcov_assemble_kernel, dim3((unsigned)G), dim3(kBlock), (sizeof(double) * 2 + sizeof(int)) * (size_t)nc, st, A.at<double>(m.o_M),
                     A.at<double>(m.o_total), A.at<double>(m.o_mu), G, p, K, rest, pb.centre ? 1 : 0, pb.standardize ? 1 : 0,
                     pb.standardize_response ? 1 : 0, A.at<double>(o_mix), A.at<double>(o_lambda), A_mix, L, A.at<double>(o_Mt),
                     A.at<double>(sets.o_scale), A.at<double>(sets.o_mean), d_tstat, A.at<double>(sets.o_pen_a), A.at<double>(sets.o_pen_b),
                     A.at<int32_t>(sets.o_ridge));
  SGD_HIP_TRY(hipGetLastError());
  SGD_HIP_TRY(hipEventRecord(ev.e[2], st));
  if (tap) {
    SGD_HIP_TRY(m.tap_cv(A, tap, pb.train_on_rest, st));
    SGD_HIP_TRY(tap_f64(tap, "Mt", A.at<double>(o_Mt), (size_t)G * (size_t)p * (size_t)nc, st));
    SGD_HIP_TRY(sets.tap(A, tap, st));
  }
  const auto kernel = width == kMcovNarrow ? cov_group_path_kernel<kMcovNarrow> : cov_group_path_kernel<kMcovWide>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)sets.jobs), dim3((unsigned)width), 0, st, A.at<double>(o_Mt), A.at<double>(sets.o_scale), p, K, G, 0.0,
                     d_tstat, A.at<double>(sets.o_pen_a), A.at<double>(sets.o_pen_b), L, 0, A.at<int32_t>(sets.o_ridge), pb.max_iter, pb.tol,
                     A.at<double>(po.o_W), A.at<double>(po.o_G), A.at<double>(po.o_c), A.at<int32_t>(po.o_sweeps), A.at<int32_t>(po.o_unconv));
  SGD_HIP_TRY(hipGetLastError());
  SGD_HIP_TRY(hipEventRecord(ev.e[3], st));
  std::vector<double> tstat;
  SGD_HIP_TRY(po.fetch(A, tap, pb.tol, pb.max_iter, out, st));
  SGD_HIP_TRY(sets.fetch(A, out, &tstat, st));
  SGD_HIP_TRY(hipStreamSynchronize(st));
  sets.split(tstat, &out->n_train, &out->yy, &out->nulldev);
  SGD_HIP_TRY(hipEventElapsedTime(&out->moments_ms, ev.e[0], ev.e[1]));
  SGD_HIP_TRY(hipEventElapsedTime(&out->assemble_ms, ev.e[1], ev.e[2]));
  SGD_HIP_TRY(hipEventElapsedTime(&out->path_ms, ev.e[2], ev.e[3]));
  return SGDNET_OK;
}

// mcovariance_cv_run beyond mcov_max_features(K) features: the same group moments pass (the wide mode's row chunks),
// wmcov_cv_stats_kernel and wmcov_cv_assemble_kernel instead of mcov_assemble_kernel, cov_wide_group_cv_path_kernel over
// the jobs.
int wmcovariance_cv_run(const McovarianceCvProblem& pb, McovarianceCvResult* out, int width, CovTap* tap) {
  const int64_t n = pb.n;
  const int K = pb.K;
  const bool sparse = pb.x_dense == nullptr;
  if (n <= 0 || pb.p <= 0 || K < 1 || pb.p > wmcov_max_features(K) || pb.n_lambda <= 0 || pb.n_groups <= 0 || pb.n_mix <= 0 || !pb.fold ||
      !pb.y || !pb.mix || !pb.lambda || (pb.train_on_rest && pb.n_groups < 2) || (!sparse && pb.colptr) ||
      (sparse && (!pb.colptr || !pb.rowidx || !pb.values))) {
    set_error("wmcovariance_cv_run: invalid problem");
    return SGDNET_EINVAL;
  }
  const int p = (int)pb.p, nc = p + K, Pa = nc + 1, L = pb.n_lambda, G = pb.n_groups, A_mix = pb.n_mix;
  if (width == 0) width = wmcov_path_width(p);
  if (width != kWideNarrow && width != kWideFull) {
    set_error("wmcovariance_cv_run: the path kernel's workgroup is %d or %d lanes, not %d", kWideNarrow, kWideFull, width);
    return SGDNET_EINVAL;
  }
  const size_t pK = (size_t)p * (size_t)K;
  GroupRows rows;
  if (!sparse)
    if (const int rc = cv_group_rows("wmcovariance", pb.fold, n, G, Pa, true, &rows)) return rc;
  if (G > kCovMaxRowChunks) {       // (the pair kernel's gridDim.z, the assembly's gridDim.y)
    set_error("mode = wmcovariance needs at most %d groups: %d groups", kCovMaxRowChunks, G);
    return SGDNET_EUNSUPPORTED;
  }
  if (wmcov_cv_bytes(G, p, K, (int64_t)rows.chunks()) > kWcovCvBytes) {
    set_error("mode = wmcovariance needs the moments and the scaled matrices of the groups within %zu bytes: %d groups of %d features and %d responses are %zu bytes",
              kWcovCvBytes, G, p, K, wmcov_cv_bytes(G, p, K, (int64_t)rows.chunks()));
    return SGDNET_EUNSUPPORTED;
  }
  SGD_HIP_TRY(hipSetDevice(pb.device));
  const int ld = (int)wide_leading_dim(p), rest = pb.train_on_rest ? 1 : 0;

  Arena A;
  Moments m(pb, K, true, true, G, pb.fold, &rows);      // (Pa^2 fits cov_total_kernel's int: covariance.hpp)
  m.reserve(A);
  const size_t o_mix = m.param(A, pb.mix, (size_t)A_mix), o_lambda = m.param(A, pb.lambda, (size_t)A_mix * (size_t)L);
  const size_t o_s = A.reserve(sizeof(double) * (size_t)G * (size_t)nc);
  const size_t o_d = A.reserve(sizeof(double) * (size_t)G * (size_t)nc);
  const size_t o_cst = A.reserve(sizeof(int32_t) * (size_t)G * (size_t)nc);
  const size_t o_S = A.reserve(sizeof(double) * (size_t)G * (size_t)ld * (size_t)p);
  const size_t o_Sd = A.reserve(sizeof(double) * (size_t)G * (size_t)p);
  const size_t o_ct = A.reserve(sizeof(double) * (size_t)G * pK);
  const size_t o_ysd = A.reserve(sizeof(double) * (size_t)G * (size_t)K);
  const CvSets sets(A, G, A_mix, L, p, nc);      // (pen_a: the l2 strengths, pen_b: the group thresholds)
  const PathOut po(A, sets.jobs, L, pK, false);
  SGD_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&A.base), A.used));

  Events ev;
  SGD_HIP_TRY(ev.open());
  hipStream_t st = ev.st;
  double* d_Mg = A.at<double>(m.o_M);
  double* d_total = A.at<double>(m.o_total);
  double* d_tstat = A.at<double>(sets.o_tstat);
  SGD_HIP_TRY(m.upload(A, st));
  SGD_HIP_TRY(hipEventRecord(ev.e[0], st));
  m.launch_cv(A, st);
  if (rest) m.launch_total(A, st);
  SGD_HIP_TRY(hipGetLastError());
  SGD_HIP_TRY(hipEventRecord(ev.e[1], st));
  hipLaunchKernelGGL(wmcov_cv_stats_kernel, dim3((unsigned)G), dim3(kBlock), 0, st, d_Mg, d_total, A.at<double>(m.o_mu), G, p, K, rest,
                     pb.centre ? 1 : 0, pb.standardize ? 1 : 0, pb.standardize_response ? 1 : 0, A.at<double>(o_mix), A.at<double>(o_lambda),
                     A_mix, L, A.at<double>(o_s), A.at<double>(o_d), A.at<int32_t>(o_cst), A.at<double>(sets.o_scale), A.at<double>(sets.o_mean),
                     A.at<double>(o_ysd), d_tstat, A.at<double>(sets.o_pen_a), A.at<double>(sets.o_pen_b), A.at<int32_t>(sets.o_ridge));
  hipLaunchKernelGGL(wmcov_cv_assemble_kernel, dim3((unsigned)p, (unsigned)G), dim3(kBlock), 0, st, d_Mg, d_total, A.at<double>(o_s),
                     A.at<double>(o_d), A.at<int32_t>(o_cst), A.at<double>(sets.o_scale), A.at<double>(o_ysd), d_tstat, p, K, ld, rest,
                     A.at<double>(o_S), A.at<double>(o_Sd), A.at<double>(o_ct));
  SGD_HIP_TRY(hipGetLastError());
  SGD_HIP_TRY(hipEventRecord(ev.e[2], st));
  if (tap) {
    SGD_HIP_TRY(m.tap_cv(A, tap, pb.train_on_rest, st));
    SGD_HIP_TRY(tap_f64(tap, "s", A.at<double>(o_s), (size_t)G * (size_t)nc, st));
    SGD_HIP_TRY(tap_f64(tap, "d", A.at<double>(o_d), (size_t)G * (size_t)nc, st));
    SGD_HIP_TRY(tap_f64(tap, "ysd", A.at<double>(o_ysd), (size_t)G * (size_t)K, st));
    SGD_HIP_TRY(sets.tap(A, tap, st));
    SGD_HIP_TRY(tap_f64(tap, "S", A.at<double>(o_S), (size_t)G * (size_t)ld * (size_t)p, st));
    SGD_HIP_TRY(tap_f64(tap, "Sd", A.at<double>(o_Sd), (size_t)G * (size_t)p, st));
    SGD_HIP_TRY(tap_f64(tap, "ct", A.at<double>(o_ct), (size_t)G * pK, st));
  }
  const auto kernel = width == kWideNarrow ? cov_wide_group_cv_path_kernel<kWideNarrow> : cov_wide_group_cv_path_kernel<kWideFull>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)sets.jobs), dim3((unsigned)width), 0, st, A.at<double>(o_S), A.at<double>(o_Sd), A.at<double>(o_ct), p,
                     K, ld, G, A.at<double>(sets.o_pen_a), A.at<double>(sets.o_pen_b), L, A.at<int32_t>(sets.o_ridge), pb.max_iter, pb.tol,
                     A.at<double>(po.o_W), A.at<double>(po.o_G), A.at<int32_t>(po.o_sweeps), A.at<int32_t>(po.o_unconv));
  SGD_HIP_TRY(hipGetLastError());
  SGD_HIP_TRY(hipEventRecord(ev.e[3], st));
  std::vector<double> tstat, ct;
  SGD_HIP_TRY(po.fetch(A, tap, pb.tol, pb.max_iter, out, st));
  SGD_HIP_TRY(sets.fetch(A, out, &tstat, st));
  SGD_HIP_TRY(download(A, o_ct, (size_t)G * pK, &ct, st));
  SGD_HIP_TRY(hipStreamSynchronize(st));
  copy_to_jobs(ct, (size_t)G, pK, &out->c);
  sets.split(tstat, &out->n_train, &out->yy, &out->nulldev);
  SGD_HIP_TRY(hipEventElapsedTime(&out->moments_ms, ev.e[0], ev.e[1]));
  SGD_HIP_TRY(hipEventElapsedTime(&out->assemble_ms, ev.e[1], ev.e[2]));
  SGD_HIP_TRY(hipEventElapsedTime(&out->path_ms, ev.e[2], ev.e[3]));
  return SGDNET_OK;
}

}  // namespace sgdnet

extern "C" int sgdnet_covariance_max_features(void) { return sgdnet::kCovMaxFeatures; }
extern "C" int sgdnet_wcovariance_max_features(void) { return sgdnet::kWcovMaxFeatures; }
extern "C" int sgdnet_mcovariance_max_features(int n_responses) { return sgdnet::mcov_max_features(n_responses); }
extern "C" int sgdnet_wmcovariance_max_features(int n_responses) { return sgdnet::wmcov_max_features(n_responses); }
