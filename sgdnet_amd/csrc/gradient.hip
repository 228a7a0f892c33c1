// The averaged loss gradient at every lambda of a fitted path (sgdnet_gradient_sparse / _dense):
//   G[k, j, l] = (1/n) sum_i x_ij r_ik(l),   G0[k, l] = (1/n) sum_i r_ik(l),
// r_i(l) the family's Gradient (device_math.hpp; reference src/families.h) at a0[:, l] + beta[:, :, l]' x_i, on x and
// y as they came: what an optimality (KKT) check of a path needs from the data, in one pass over x per chunk of
// lambdas (sgdnet_amd/kkt.py turns it into residuals in the driver's units).
//
// Two kernels per chunk of lambdas:
//   residual_kernel   a wavefront owns a sample, lane c the (lambda, class) pair c of the chunk, as score_kernel
//                     does (the same pair chunking and relayout_beta_kernel, path_pairs.hpp); the residuals go to
//                     R[i * Cs + c], pair-fastest, Cs = the chunk's pairs rounded up to kTile (the padding is 0).
//                     exp / log are the plain-IEEE ones of include/sgdnet_detmath.h, as in the exact kernels.
//   colreduce_kernel  a group of kGroup lanes (64: a wavefront; 16 for short columns) owns one feature column and
//                     one tile of kTile pairs.  Lane t takes the column's entries t, t + kGroup, ... in order and adds
//                     x_ij * R[i, tile] to kTile sums (four 128-bit loads of R per entry); the lanes' sums are then
//                     added by a butterfly (xor 32, 16, ..., 1).  Column p is the column of ones: G0.
// No floating-point atomic anywhere; which lane adds which entry, and the butterfly, depend on the column lengths and
// the group width alone, and the width is chosen from (n, p, nnz): two calls on the same input return the same bits.
//
// Memory bound: the residual block of a chunk is n * Cs doubles.  A chunk takes as many lambdas as fit kMaxPairs /
// kMaxLambda AND kResidualBytes (1 GiB), never less than one: the block is at most max(1 GiB, 8 n roundup(K, kTile))
// bytes whatever n_lambda is (config 3, 1M samples x 100 lambdas: one chunk of 0.8 GB; config 5, 50M samples x
// 10 classes: one lambda per chunk, 6.4 GB).
//
// Sparse x arrives feature-major (the dgCMatrix slots), which is what the column reduction reads; the residual
// pass reads the sample-major copy made by the fit's own device transpose (setup_device.hip device_transpose).
// Dense x is read column-major by both passes.
#define SGDNET_DET_MATH
#include <vector>

#include "common.hpp"
#include "device_math.hpp"
#include "path_pairs.hpp"
#include "setup_device.hpp"

namespace sgdnet {
namespace {

constexpr int kResBlock = 256;                       // 4 wavefronts, one sample each at a time
constexpr int kTile = 8;                             // pairs per column-reduction group: 64 B of a residual row
constexpr size_t kResidualBytes = (size_t)1 << 30;   // the residual block of a chunk (see above)

struct GradArgs {
  int64_t n, p;
  int family, K, Ky, L, Cs;
  const int64_t* sptr;     // sparse, sample-major
  const int32_t* sidx;
  const double* sval;
  const int32_t* colptr;   // sparse, feature-major
  const int32_t* rowidx;
  const double* val;
  const double* xd;        // dense, column-major n x p
  const double* y;         // Ky x n
  const double* a0;        // K x L of the chunk
  const double* B;         // p x L x K
  double* R;               // n x Cs
  double* G;               // the chunk's K x p x L slice of the output
  double* G0;              // the chunk's K x L slice
};

template <bool kSparse>
__global__ __launch_bounds__(kResBlock) void residual_kernel(GradArgs a) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int K = a.K, LK = a.L * a.K;
  double* lp = lds + (size_t)wave * (LK + a.L);     // the wave's own rows: LK linear predictors, L log-sum-exps
  double* lse = lp + LK;
  const int64_t wave_id = (int64_t)blockIdx.x * (kResBlock / 64) + wave;
  const int64_t n_waves = (int64_t)gridDim.x * (kResBlock / 64);
  for (int64_t i = wave_id; i < a.n; i += n_waves) {
    for (int c0 = 0; c0 < LK; c0 += 64) {
      const int c = c0 + lane;
      const bool on = c < LK;
      double acc = 0.0;
      if (kSparse) {
        const int64_t q1 = a.sptr[i + 1];
        for (int64_t q = a.sptr[i]; q < q1; ++q) {
          const double v = a.sval[q];
          const int64_t j = a.sidx[q];
          if (on) acc += v * a.B[j * LK + c];
        }
      } else {
        for (int64_t j = 0; j < a.p; ++j) {
          const double v = a.xd[i + j * a.n];
          if (on && v != 0.0) acc += v * a.B[j * LK + c];
        }
      }
      if (on) lp[c] = acc + a.a0[c];
    }
    // the wave's own LDS rows: LDS operations of one wave are served in issue order; the fences keep the
    // compiler from moving the reads above the writes
    __threadfence_block();
    const double* ys = a.y + i * a.Ky;
    if (a.family == SGDNET_MULTINOMIAL) {           // one LogSumExp per lambda, not one per pair
      for (int l = lane; l < a.L; l += 64) lse[l] = log_sum_exp(lp + (size_t)l * K, K);
      __threadfence_block();
    }
    double* Ri = a.R + i * a.Cs;
    for (int c0 = 0; c0 < a.Cs; c0 += 64) {
      const int c = c0 + lane;
      if (c >= a.Cs) break;
      double g = 0.0;                               // the padding of the row
      if (c < LK) {
        const int l = c / K, k = c - l * K;
        if (a.family == SGDNET_MULTINOMIAL) {       // family_gradient_k with the shared LogSumExp
          g = SGD_EXP(lp[c] - lse[l]);
          if ((unsigned)k == (unsigned)(ys[0] + 0.5)) g -= 1.0;
        } else {
          g = family_gradient_k(a.family, K, k, lp + (size_t)l * K, ys);
        }
      }
      Ri[c] = g;
    }
    __threadfence_block();
  }
}

// blockIdx.x: 256 / kGroup columns (column p: the ones), blockIdx.y: the tile of pairs
template <bool kSparse, int kGroup>
__global__ __launch_bounds__(256) void colreduce_kernel(GradArgs a) {
  const int t = threadIdx.x & (kGroup - 1);
  const int64_t j = (int64_t)blockIdx.x * (256 / kGroup) + threadIdx.x / kGroup;
  const int c0 = (int)blockIdx.y * kTile;
  double s[kTile];
#pragma unroll
  for (int u = 0; u < kTile; ++u) s[u] = 0.0;
  if (j <= a.p) {
    const bool ones = j == a.p;
    int64_t q0 = 0, q1 = a.n;
    if (kSparse && !ones) {
      q0 = a.colptr[j];
      q1 = a.colptr[j + 1];
    }
    const double* col = kSparse ? a.val : a.xd + j * a.n;
    for (int64_t q = q0 + t; q < q1; q += kGroup) {
      const int64_t i = (kSparse && !ones) ? (int64_t)a.rowidx[q] : q;
      const double v = ones ? 1.0 : col[q];
      const double2* r = reinterpret_cast<const double2*>(a.R + i * a.Cs + c0);   // 64-B aligned: Cs, c0 multiples of kTile
#pragma unroll
      for (int u = 0; u < kTile / 2; ++u) {
        const double2 rr = r[u];
        s[2 * u] += v * rr.x;
        s[2 * u + 1] += v * rr.y;
      }
    }
  }
  // every lane of the wavefront takes part in the butterfly (columns past p carry zeros); offsets below kGroup
  // stay inside the group
#pragma unroll
  for (int u = 0; u < kTile; ++u)
    for (int off = kGroup / 2; off > 0; off >>= 1) s[u] += __shfl_xor(s[u], off, 64);
  if (t == 0 && j <= a.p) {
    const int K = a.K, LK = a.L * a.K;
    const double nn = (double)a.n;
#pragma unroll
    for (int u = 0; u < kTile; ++u) {
      const int c = c0 + u;
      if (c >= LK) break;
      const int l = c / K, k = c - l * K;
      if (j == a.p) a.G0[k + (int64_t)K * l] = s[u] / nn;
      else a.G[k + (int64_t)K * (j + a.p * l)] = s[u] / nn;
    }
  }
}

struct DevBufs {
  std::vector<void*> all;
  ~DevBufs() {
    for (void* q : all) (void)hipFree(q);
  }
  template <typename T>
  int upload(T** out, const T* host, size_t count, hipStream_t st) {
    void* q = nullptr;
    if (hipMalloc(&q, sizeof(T) * (count ? count : 1)) != hipSuccess) {
      set_error("hipMalloc(%zu bytes) failed", sizeof(T) * count);
      return SGDNET_ENOMEM;
    }
    all.push_back(q);
    if (host && count) SGD_HIP_TRY(hipMemcpyAsync(q, host, sizeof(T) * count, hipMemcpyHostToDevice, st));
    *out = static_cast<T*>(q);
    return SGDNET_OK;
  }
};

int run_gradient(const sgdnet_csc* xs, const double* xd, int64_t n, int64_t p, const double* y, int y_cols, int family,
                 int n_classes, const double* a0, const double* beta, int n_lambda, int device, double* G, double* G0) {
  if (n < 1 || p < 1 || n_lambda < 1 || n_classes < 1 || !y || !a0 || !beta || !G || !G0 ||
      family < SGDNET_GAUSSIAN || family > SGDNET_MGAUSSIAN || (!xd && !xs) ||
      (xs && (!xs->colptr || !xs->rowidx || !xs->values)) ||
      y_cols != (family == SGDNET_MGAUSSIAN ? n_classes : 1) ||
      ((family == SGDNET_GAUSSIAN || family == SGDNET_BINOMIAL) && n_classes != 1)) {
    set_error("sgdnet_gradient: bad argument");
    return SGDNET_EINVAL;
  }
  const int K = n_classes, Ky = y_cols;
  if (family == SGDNET_BINOMIAL || family == SGDNET_MULTINOMIAL) {
    const double top = family == SGDNET_BINOMIAL ? 1.0 : (double)(K - 1);
    for (int64_t i = 0; i < n; ++i)
      if (!(y[i] >= 0.0 && y[i] <= top && y[i] == floor(y[i]))) {
        set_error("response[%lld] = %g is not a class code in 0..%d", (long long)i, y[i], (int)top);
        return SGDNET_EINVAL;
      }
  }
  int64_t nnz = 0;
  if (xs) {                                        // the checks of sgdnet_fit_sparse: the kernels index with these
    if (xs->colptr[0] != 0) {
      set_error("colptr[0] must be 0");
      return SGDNET_EINVAL;
    }
    for (int64_t j = 0; j < p; ++j)
      if (xs->colptr[j + 1] < xs->colptr[j]) {
        set_error("colptr is not non-decreasing at column %lld", (long long)j);
        return SGDNET_EINVAL;
      }
    nnz = xs->colptr[p];
    for (int64_t q = 0; q < nnz; ++q)
      if (xs->rowidx[q] < 0 || xs->rowidx[q] >= n) {
        set_error("row index %d out of range at position %lld", xs->rowidx[q], (long long)q);
        return SGDNET_EINVAL;
      }
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    set_error("no HIP device");
    return SGDNET_ENODEVICE;
  }
  if (device < 0 || device >= ndev) {
    set_error("device %d out of range (%d devices)", device, ndev);
    return SGDNET_EINVAL;
  }
  // lambdas per chunk: the pair chunking of sgdnet_score_*, and the bound on the residual block
  int chunk = kMaxPairs / K;
  if (chunk > kMaxLambda) chunk = kMaxLambda;
  if (chunk < 1) {
    set_error("sgdnet_gradient: more than %d classes", kMaxPairs);
    return SGDNET_EUNSUPPORTED;
  }
  {
    const size_t row_bytes = sizeof(double) * (size_t)n * (size_t)K;
    const size_t fit = kResidualBytes / row_bytes;
    if ((size_t)chunk > fit) chunk = fit < 1 ? 1 : (int)fit;
  }
  if (chunk > n_lambda) chunk = n_lambda;
  const int Cs_max = (chunk * K + kTile - 1) / kTile * kTile;

  SGD_HIP_TRY(hipSetDevice(device));
  hipStream_t st = nullptr;
  SGD_HIP_TRY(hipStreamCreate(&st));
  struct Guard {
    hipStream_t s;
    DeviceSetup S;
    ~Guard() {
      S.release();
      (void)hipStreamDestroy(s);
    }
  } guard{st, {}};
  DevBufs bufs;
  GradArgs a{};
  a.n = n;
  a.p = p;
  a.family = family;
  a.K = K;
  a.Ky = Ky;
  int rc;
  if (xd) {
    double* x_d;
    if ((rc = bufs.upload(&x_d, xd, (size_t)n * p, st))) return rc;
    a.xd = x_d;
  } else {
    DeviceSetup& S = guard.S;
    S.n = n;
    S.p = p;
    S.nnz = nnz;
    if ((rc = bufs.upload(&S.colptr, xs->colptr, (size_t)p + 1, st)) || (rc = bufs.upload(&S.rowidx, xs->rowidx, (size_t)nnz, st)) ||
        (rc = bufs.upload(&S.val, xs->values, (size_t)nnz, st)))
      return rc;
    a.colptr = S.colptr;
    a.rowidx = S.rowidx;
    a.val = S.val;
    rc = device_transpose(S, st);
    S.colptr = S.rowidx = nullptr;                 // bufs owns the feature-major copy; S the sample-major one
    S.val = nullptr;
    if (rc) return rc;
    a.sptr = S.sptr;
    a.sidx = S.sidx;
    a.sval = S.sval;
  }
  std::vector<double> yt((size_t)n * Ky);          // Ky x n, as the solvers read it (src/sgdnet.cpp:178)
  for (int64_t i = 0; i < n; ++i)
    for (int k = 0; k < Ky; ++k) yt[(size_t)(k + i * Ky)] = y[i + (int64_t)k * n];
  double *y_d, *beta_d, *a0_d, *B, *R, *G_d, *G0_d;
  const size_t Kz = (size_t)K;
  if ((rc = bufs.upload(&y_d, yt.data(), yt.size(), st)) || (rc = bufs.upload(&beta_d, beta, Kz * p * n_lambda, st)) ||
      (rc = bufs.upload(&a0_d, a0, Kz * n_lambda, st)) || (rc = bufs.upload<double>(&B, nullptr, Kz * p * chunk, st)) ||
      (rc = bufs.upload<double>(&R, nullptr, (size_t)n * Cs_max, st)) ||
      (rc = bufs.upload<double>(&G_d, nullptr, Kz * p * n_lambda, st)) ||
      (rc = bufs.upload<double>(&G0_d, nullptr, Kz * n_lambda, st)))
    return rc;
  a.y = y_d;
  a.B = B;
  a.R = R;
  int64_t grid = (n + 3) / 4;
  if (grid > 8192) grid = 8192;
  // short columns: four to a wavefront (the ones column and dense columns have n entries)
  const bool narrow = xd ? n <= 32 : nnz <= 32 * p;
  for (int l0 = 0; l0 < n_lambda; l0 += chunk) {
    const int L = n_lambda - l0 < chunk ? n_lambda - l0 : chunk;
    int rgrid = (int)((Kz * p * L + 255) / 256);
    if (rgrid > 4096) rgrid = 4096;
    hipLaunchKernelGGL(relayout_beta_kernel, dim3(rgrid), dim3(256), 0, st, beta_d + Kz * p * l0, p, K, L, B);
    a.L = L;
    a.Cs = (L * K + kTile - 1) / kTile * kTile;
    a.a0 = a0_d + Kz * l0;
    a.G = G_d + Kz * p * l0;
    a.G0 = G0_d + Kz * l0;
    const size_t lds = sizeof(double) * (size_t)(kResBlock / 64) * (size_t)(L * K + L);
    if (xd)
      hipLaunchKernelGGL(residual_kernel<false>, dim3((unsigned)grid), dim3(kResBlock), lds, st, a);
    else
      hipLaunchKernelGGL(residual_kernel<true>, dim3((unsigned)grid), dim3(kResBlock), lds, st, a);
    SGD_HIP_TRY(hipGetLastError());
    const int per_block = narrow ? 16 : 4;
    const dim3 cgrid((unsigned)((p + 1 + per_block - 1) / per_block), (unsigned)(a.Cs / kTile));
    if (xd) {
      if (narrow) hipLaunchKernelGGL((colreduce_kernel<false, 16>), cgrid, dim3(256), 0, st, a);
      else hipLaunchKernelGGL((colreduce_kernel<false, 64>), cgrid, dim3(256), 0, st, a);
    } else {
      if (narrow) hipLaunchKernelGGL((colreduce_kernel<true, 16>), cgrid, dim3(256), 0, st, a);
      else hipLaunchKernelGGL((colreduce_kernel<true, 64>), cgrid, dim3(256), 0, st, a);
    }
    SGD_HIP_TRY(hipGetLastError());
  }
  SGD_HIP_TRY(hipMemcpyAsync(G, G_d, sizeof(double) * Kz * p * n_lambda, hipMemcpyDeviceToHost, st));
  SGD_HIP_TRY(hipMemcpyAsync(G0, G0_d, sizeof(double) * Kz * n_lambda, hipMemcpyDeviceToHost, st));
  SGD_HIP_TRY(hipStreamSynchronize(st));
  return SGDNET_OK;
}

}  // namespace
}  // namespace sgdnet

extern "C" {

int sgdnet_gradient_sparse(const sgdnet_csc* x, const double* y, int y_cols, int family, int n_classes,
                           const double* a0, const double* beta, int n_lambda, int device, double* G, double* G0) {
  if (!x) {
    sgdnet::set_error("sgdnet_gradient_sparse: no matrix");
    return SGDNET_EINVAL;
  }
  return sgdnet::run_gradient(x, nullptr, x->n_rows, x->n_cols, y, y_cols, family, n_classes, a0, beta, n_lambda, device, G, G0);
}

int sgdnet_gradient_dense(const double* x, int64_t n, int64_t p, const double* y, int y_cols, int family,
                          int n_classes, const double* a0, const double* beta, int n_lambda, int device,
                          double* G, double* G0) {
  if (!x) {
    sgdnet::set_error("sgdnet_gradient_dense: no matrix");
    return SGDNET_EINVAL;
  }
  return sgdnet::run_gradient(nullptr, x, n, p, y, y_cols, family, n_classes, a0, beta, n_lambda, device, G, G0);
}

}  // extern "C"
