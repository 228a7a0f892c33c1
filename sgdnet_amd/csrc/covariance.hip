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
// No floating-point atomic anywhere and every reduction in an order fixed by (n, p, nnz): the same input gives the
// same bits (the contract of gradient.hip).
#include <algorithm>
#include <numeric>
#include <vector>

#include "common.hpp"
#include "covariance.hpp"

namespace sgdnet {
namespace {

constexpr int kBlock = 256;
constexpr int kTileCols = 16;     // columns per tile: 16 x 16 threads own a tile pair
constexpr int kTileRows = 64;     // rows staged per step

// the sum of v over the workgroup, in a fixed tree order; every thread gets it
__device__ double block_sum(double v, double* sh) {
  __syncthreads();
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  return sh[0];
}

// blockIdx.x = column j < p: mu[j] = mean of the column (sparse: over all n samples); column p: mu[p] = sum of y
template <bool kSparse>
__global__ __launch_bounds__(kBlock) void cov_sum_kernel(const double* __restrict__ x, const int32_t* __restrict__ colptr,
                                                          const double* __restrict__ y, int64_t n, int p, int centre,
                                                          double* __restrict__ mu) {
  __shared__ double sh[kBlock];
  const int j = blockIdx.x;
  double s = 0.0;
  if (j == p) {
    for (int64_t i = threadIdx.x; i < n; i += kBlock) s += y[i];
  } else if (!centre) {
    // deviations from 0
  } else if (kSparse) {
    for (int64_t q = (int64_t)colptr[j] + threadIdx.x; q < colptr[j + 1]; q += kBlock) s += x[q];
  } else {
    const double* col = x + (int64_t)j * n;
    for (int64_t i = threadIdx.x; i < n; i += kBlock) s += col[i];
  }
  s = block_sum(s, sh);
  if (threadIdx.x == 0) mu[j] = j == p ? s : s / (double)n;
}

// blockIdx.x: the pair (tj <= tk) of column tiles of the augmented matrix [x - mu | y], blockIdx.y: the chunk of rows
__global__ __launch_bounds__(kBlock) void cov_dense_tile_kernel(const double* __restrict__ x, const double* __restrict__ y,
                                                                 const double* __restrict__ mu, int64_t n, int p,
                                                                 int64_t rows_per_chunk, double* __restrict__ part) {
  __shared__ double A[kTileCols][kTileRows + 1], B[kTileCols][kTileRows + 1];
  const int tid = threadIdx.x;
  const int T = (p + 1 + kTileCols - 1) / kTileCols;
  int pair = blockIdx.x, tj = 0;
  while (pair >= T - tj) {
    pair -= T - tj;
    ++tj;
  }
  const int tk = tj + pair;
  const int ta = tid & (kTileCols - 1), tb = tid / kTileCols;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_chunk, r1 = r0 + rows_per_chunk < n ? r0 + rows_per_chunk : n;
  auto dev = [&](int a, int64_t i) -> double {
    if (i >= r1 || a > p) return 0.0;
    return a < p ? x[i + (int64_t)a * n] - mu[a] : y[i];
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

// the chunks' partial tiles added in chunk order; M is the symmetric (p + 1) x (p + 1) matrix of [x - mu | y]
__global__ __launch_bounds__(kBlock) void cov_reduce_kernel(const double* __restrict__ part, int chunks, int p,
                                                             double* __restrict__ M) {
  const int tid = threadIdx.x, P1 = p + 1;
  const int T = (P1 + kTileCols - 1) / kTileCols;
  int pair = blockIdx.x, tj = 0;
  while (pair >= T - tj) {
    pair -= T - tj;
    ++tj;
  }
  const int tk = tj + pair;
  const int a = tj * kTileCols + (tid & (kTileCols - 1)), b = tk * kTileCols + tid / kTileCols;
  if (a >= P1 || b >= P1) return;
  double s = 0.0;
  for (int c = 0; c < chunks; ++c) s += part[((size_t)c * gridDim.x + blockIdx.x) * kBlock + tid];
  M[(size_t)a * P1 + b] = s;
  if (tj != tk) M[(size_t)b * P1 + a] = s;
}

// first position in rowidx[lo, hi) whose row is >= r
__device__ int lower_bound_row(const int32_t* __restrict__ rowidx, int lo, int hi, int32_t r) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (rowidx[mid] < r) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// blockIdx.x = column j < p, blockIdx.y = column k in [j, p]; k == p is the response
__global__ __launch_bounds__(kBlock) void cov_sparse_pair_kernel(const int32_t* __restrict__ colptr, const int32_t* __restrict__ rowidx,
                                                                  const double* __restrict__ val, const double* __restrict__ y,
                                                                  const double* __restrict__ mu, int64_t n, int p,
                                                                  double* __restrict__ M) {
  __shared__ double sh[kBlock];
  const int j = blockIdx.x, k = blockIdx.y, P1 = p + 1, tid = threadIdx.x;
  if (k < j) return;
  const int q0 = colptr[j], q1 = colptr[j + 1];
  const double mj = mu[j];
  if (k == p) {
    double a = 0.0, ys = 0.0;
    for (int q = q0 + tid; q < q1; q += kBlock) {
      const double yi = y[rowidx[q]];
      a += (val[q] - mj) * yi;
      ys += yi;
    }
    a = block_sum(a, sh);
    ys = block_sum(ys, sh);
    if (tid == 0) {
      const double rest = (int64_t)(q1 - q0) == n ? 0.0 : mu[p] - ys;     // the response over the samples NOT stored: none, or all - stored
      const double c = a - mj * rest;
      M[(size_t)j * P1 + p] = c;
      M[(size_t)p * P1 + j] = c;
    }
    return;
  }
  const int s0 = colptr[k], s1 = colptr[k + 1];
  const double mk = mu[k];
  double both = 0.0, only_j = 0.0, only_k = 0.0, cnt = 0.0;
  for (int q = q0 + tid; q < q1; q += kBlock) {
    const int32_t r = rowidx[q];
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
      const int pos = lower_bound_row(rowidx, q0, q1, r);
      if (!(pos < q1 && rowidx[pos] == r)) only_k += val[s] - mk;
    }
  both = block_sum(both, sh);
  only_j = block_sum(only_j, sh);
  only_k = block_sum(only_k, sh);
  cnt = block_sum(cnt, sh);
  if (tid == 0) {
    const double in_neither = (double)n - ((double)(q1 - q0) + (double)(s1 - s0) - cnt);
    const double c = both - mk * only_j - mj * only_k + in_neither * mj * mk;
    M[(size_t)j * P1 + k] = c;
    M[(size_t)k * P1 + j] = c;
  }
}

// S(j, k) of the packed triangle, j <= k
__device__ __forceinline__ int tri(int j, int k) { return k * (k + 1) / 2 + j; }

// One wavefront, the whole path.  Every lane computes the sweep's scalars (the new coefficient, the sweep's
// max|dw| and max|w|) from the same LDS words, so branches on them are uniform and nothing has to be broadcast.
__global__ __launch_bounds__(64) void cov_path_kernel(const double* __restrict__ M, const double* __restrict__ scale, int p, double dn,
                                                       const double* __restrict__ alpha, const double* __restrict__ beta, int n_lambda,
                                                       int ridge, unsigned max_iter, double tol, double* __restrict__ W,
                                                       double* __restrict__ G, double* __restrict__ c_out, int32_t* __restrict__ sweeps_out,
                                                       int32_t* __restrict__ unconverged) {
  __shared__ double lds[cov_state_doubles(kCovMaxFeatures)];
  const int lane = threadIdx.x, P1 = p + 1;
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

// one device allocation cut into aligned pieces
struct Arena {
  char* base = nullptr;
  size_t used = 0;
  ~Arena() {
    if (base) (void)hipFree(base);
  }
  size_t reserve(size_t bytes) {
    const size_t at = used;
    used += (bytes + 255) & ~(size_t)255;
    return at;
  }
  template <class T>
  T* at(size_t off) const { return reinterpret_cast<T*>(base + off); }
};

struct Events {
  hipEvent_t e[3] = {nullptr, nullptr, nullptr};
  hipStream_t st = nullptr;
  ~Events() {
    for (hipEvent_t v : e)
      if (v) (void)hipEventDestroy(v);
    if (st) (void)hipStreamDestroy(st);
  }
};

}  // namespace

int covariance_run(const CovarianceProblem& pb, CovarianceResult* out) {
  const int64_t n = pb.n;
  const int p = (int)pb.p, P1 = p + 1, L = pb.n_lambda;
  const bool sparse = pb.x_dense == nullptr;
  if (n <= 0 || p <= 0 || p > kCovMaxFeatures || L <= 0 || (!sparse && pb.colptr) || (sparse && (!pb.colptr || !pb.rowidx || !pb.values))) {
    set_error("covariance_run: invalid problem");
    return SGDNET_EINVAL;
  }
  SGD_HIP_TRY(hipSetDevice(pb.device));

  // the pair kernel looks rows up by binary search: columns whose row indices do not ascend are sorted in a copy
  const int64_t nnz = sparse ? pb.colptr[p] : 0;
  const int32_t* rowidx = pb.rowidx;
  const double* values = pb.values;
  std::vector<int32_t> rows_sorted;
  std::vector<double> vals_sorted;
  if (sparse) {
    bool ascending = true;
    for (int j = 0; j < p && ascending; ++j)
      for (int64_t q = (int64_t)pb.colptr[j] + 1; q < pb.colptr[j + 1]; ++q)
        if (rowidx[q] <= rowidx[q - 1]) {
          ascending = false;
          break;
        }
    if (!ascending) {
      rows_sorted.assign(rowidx, rowidx + nnz);
      vals_sorted.assign(values, values + nnz);
      std::vector<int64_t> order;
      for (int j = 0; j < p; ++j) {
        const int64_t q0 = pb.colptr[j], q1 = pb.colptr[j + 1];
        order.resize((size_t)(q1 - q0));
        std::iota(order.begin(), order.end(), q0);
        std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return rowidx[a] < rowidx[b]; });
        for (int64_t q = q0; q < q1; ++q) {
          rows_sorted[(size_t)q] = rowidx[order[(size_t)(q - q0)]];
          vals_sorted[(size_t)q] = values[order[(size_t)(q - q0)]];
        }
      }
      rowidx = rows_sorted.data();
      values = vals_sorted.data();
    }
  }

  // dense x: the tile pairs and the row chunks (a function of n and p alone)
  const int T = (P1 + kTileCols - 1) / kTileCols, pairs = T * (T + 1) / 2;
  const int64_t chunk_cap = std::max<int64_t>(16, std::min<int64_t>(256, 1024 / pairs));
  int64_t chunks = std::min<int64_t>(chunk_cap, (n + 255) / 256);
  const int64_t rows_per_chunk = ((n + chunks - 1) / chunks + kTileRows - 1) / kTileRows * kTileRows;
  chunks = (n + rows_per_chunk - 1) / rows_per_chunk;

  Arena A;
  const size_t o_x = A.reserve(sizeof(double) * (size_t)(sparse ? nnz : n * (int64_t)p));
  const size_t o_colptr = A.reserve(sparse ? sizeof(int32_t) * (size_t)P1 : 0);
  const size_t o_rowidx = A.reserve(sparse ? sizeof(int32_t) * (size_t)nnz : 0);
  const size_t o_y = A.reserve(sizeof(double) * (size_t)n);
  const size_t o_mu = A.reserve(sizeof(double) * (size_t)P1);
  const size_t o_scale = A.reserve(sizeof(double) * (size_t)p);
  const size_t o_part = A.reserve(sparse ? 0 : sizeof(double) * (size_t)(chunks * pairs * kBlock));
  const size_t o_M = A.reserve(sizeof(double) * (size_t)P1 * (size_t)P1);
  const size_t o_alpha = A.reserve(sizeof(double) * (size_t)L);
  const size_t o_beta = A.reserve(sizeof(double) * (size_t)L);
  const size_t o_W = A.reserve(sizeof(double) * (size_t)L * (size_t)p);
  const size_t o_G = A.reserve(sizeof(double) * (size_t)L * (size_t)p);
  const size_t o_c = A.reserve(sizeof(double) * (size_t)p);
  const size_t o_sweeps = A.reserve(sizeof(int32_t) * (size_t)L);
  const size_t o_unconv = A.reserve(sizeof(int32_t) * (size_t)L);
  SGD_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&A.base), A.used));

  Events ev;
  SGD_HIP_TRY(hipStreamCreateWithFlags(&ev.st, hipStreamNonBlocking));
  for (hipEvent_t& e : ev.e) SGD_HIP_TRY(hipEventCreate(&e));
  hipStream_t st = ev.st;
  double* d_x = A.at<double>(o_x);
  int32_t* d_colptr = A.at<int32_t>(o_colptr);
  int32_t* d_rowidx = A.at<int32_t>(o_rowidx);
  double* d_y = A.at<double>(o_y);
  double* d_mu = A.at<double>(o_mu);
  double* d_M = A.at<double>(o_M);
  if (sparse) {
    if (nnz > 0) {
      SGD_HIP_TRY(hipMemcpyAsync(d_x, values, sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice, st));
      SGD_HIP_TRY(hipMemcpyAsync(d_rowidx, rowidx, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice, st));
    }
    SGD_HIP_TRY(hipMemcpyAsync(d_colptr, pb.colptr, sizeof(int32_t) * (size_t)P1, hipMemcpyHostToDevice, st));
  } else {
    SGD_HIP_TRY(hipMemcpyAsync(d_x, pb.x_dense, sizeof(double) * (size_t)(n * (int64_t)p), hipMemcpyHostToDevice, st));
  }
  SGD_HIP_TRY(hipMemcpyAsync(d_y, pb.y, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
  SGD_HIP_TRY(hipMemcpyAsync(A.at<double>(o_scale), pb.scale, sizeof(double) * (size_t)p, hipMemcpyHostToDevice, st));
  SGD_HIP_TRY(hipMemcpyAsync(A.at<double>(o_alpha), pb.alpha, sizeof(double) * (size_t)L, hipMemcpyHostToDevice, st));
  SGD_HIP_TRY(hipMemcpyAsync(A.at<double>(o_beta), pb.beta, sizeof(double) * (size_t)L, hipMemcpyHostToDevice, st));

  SGD_HIP_TRY(hipEventRecord(ev.e[0], st));
  if (sparse) {
    hipLaunchKernelGGL(cov_sum_kernel<true>, dim3((unsigned)P1), dim3(kBlock), 0, st, d_x, d_colptr, d_y, n, p, pb.centre ? 1 : 0, d_mu);
    hipLaunchKernelGGL(cov_sparse_pair_kernel, dim3((unsigned)p, (unsigned)P1), dim3(kBlock), 0, st, d_colptr, d_rowidx, d_x, d_y,
                       d_mu, n, p, d_M);
  } else {
    hipLaunchKernelGGL(cov_sum_kernel<false>, dim3((unsigned)P1), dim3(kBlock), 0, st, d_x, (const int32_t*)nullptr, d_y, n, p,
                       pb.centre ? 1 : 0, d_mu);
    hipLaunchKernelGGL(cov_dense_tile_kernel, dim3((unsigned)pairs, (unsigned)chunks), dim3(kBlock), 0, st, d_x, d_y, d_mu, n, p,
                       rows_per_chunk, A.at<double>(o_part));
    hipLaunchKernelGGL(cov_reduce_kernel, dim3((unsigned)pairs), dim3(kBlock), 0, st, A.at<double>(o_part), (int)chunks, p, d_M);
  }
  SGD_HIP_TRY(hipGetLastError());
  SGD_HIP_TRY(hipEventRecord(ev.e[1], st));
  hipLaunchKernelGGL(cov_path_kernel, dim3(1), dim3(64), 0, st, d_M, A.at<double>(o_scale), p, (double)n, A.at<double>(o_alpha),
                     A.at<double>(o_beta), L, pb.ridge ? 1 : 0, pb.max_iter, pb.tol, A.at<double>(o_W), A.at<double>(o_G),
                     A.at<double>(o_c), A.at<int32_t>(o_sweeps), A.at<int32_t>(o_unconv));
  SGD_HIP_TRY(hipGetLastError());
  SGD_HIP_TRY(hipEventRecord(ev.e[2], st));

  out->mean.resize((size_t)P1);
  out->c.resize((size_t)p);
  out->w.resize((size_t)L * (size_t)p);
  out->g.resize((size_t)L * (size_t)p);
  out->sweeps.resize((size_t)L);
  out->unconverged.resize((size_t)L);
  SGD_HIP_TRY(hipMemcpyAsync(out->mean.data(), d_mu, sizeof(double) * (size_t)P1, hipMemcpyDeviceToHost, st));
  SGD_HIP_TRY(hipMemcpyAsync(out->c.data(), A.at<double>(o_c), sizeof(double) * (size_t)p, hipMemcpyDeviceToHost, st));
  SGD_HIP_TRY(hipMemcpyAsync(out->w.data(), A.at<double>(o_W), sizeof(double) * (size_t)L * (size_t)p, hipMemcpyDeviceToHost, st));
  SGD_HIP_TRY(hipMemcpyAsync(out->g.data(), A.at<double>(o_G), sizeof(double) * (size_t)L * (size_t)p, hipMemcpyDeviceToHost, st));
  SGD_HIP_TRY(hipMemcpyAsync(out->sweeps.data(), A.at<int32_t>(o_sweeps), sizeof(int32_t) * (size_t)L, hipMemcpyDeviceToHost, st));
  SGD_HIP_TRY(hipMemcpyAsync(out->unconverged.data(), A.at<int32_t>(o_unconv), sizeof(int32_t) * (size_t)L, hipMemcpyDeviceToHost, st));
  SGD_HIP_TRY(hipStreamSynchronize(st));
  out->mean.resize((size_t)p);     // (entry p was the response's sum)
  SGD_HIP_TRY(hipEventElapsedTime(&out->moments_ms, ev.e[0], ev.e[1]));
  SGD_HIP_TRY(hipEventElapsedTime(&out->path_ms, ev.e[1], ev.e[2]));
  return SGDNET_OK;
}

}  // namespace sgdnet

extern "C" int sgdnet_covariance_max_features(void) { return sgdnet::kCovMaxFeatures; }
