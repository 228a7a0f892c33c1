// Multinomial Newton mode (SGDNET_MODE_MNEWTON): what the plan, the driver and mnewton.hip share.
// No HIP type in here: fit_plan.hpp includes this file for the feature limit.
#pragma once

#include <stdint.h>

#include <vector>

#include "newton.hpp"

namespace sgdnet {

// The inner solve (mnewton.hip: mnewton_cd_kernel) is ONE workgroup that keeps, in f64, for one outer step over the
// Q = K (p + 1) coordinates U = (w_k, b_k), k = 1 .. K -- coordinate (k, j) at k (p + 1) + j, the intercept j = p --
//   the joint Hessian as a packed triangle              Q (Q + 1) / 2
//   U and the running gradient g = H (U - U0) - q        2 Q
//   nothing else (the sweep's reductions live in registers, as in newton_cd_kernel)
// in its LDS, out of the budget of newton.hpp (160 KiB = 20 480 doubles):
//   Q = 199:  19 900 + 398 = 20 298 <= 20 480          Q = 200:  20 100 + 400 = 20 500 > 20 480
// so K classes leave room for 199 / K - 1 features: 98 at K = 2, 65 at K = 3, 48 at K = 4, 38 at K = 5, 18 at K = 10,
// 1 at K = 99 and none from K = 100 on (K < 2 is not a multinomial problem).
constexpr int mnewton_state_doubles(int Q) { return Q * (Q + 1) / 2 + 2 * Q; }
constexpr int mnewton_max_coordinates() {
  int Q = 1;
  while (mnewton_state_doubles(Q + 1) <= kNewtonLdsDoubles) ++Q;
  return Q;
}
constexpr int kMNewtonMaxCoordinates = mnewton_max_coordinates();
static_assert(kMNewtonMaxCoordinates == 199, "the LDS budget of the inner solve (see above)");
constexpr int mnewton_max_features(int K) {
  if (K < 2 || K > kMNewtonMaxCoordinates) return 0;
  const int p = kMNewtonMaxCoordinates / K - 1;
  return p > 0 ? p : 0;
}
static_assert(mnewton_max_features(2) == 98 && mnewton_max_features(3) == 65 && mnewton_max_features(4) == 48, "the LDS budget (see above)");
static_assert(mnewton_max_features(5) == 38 && mnewton_max_features(10) == 18 && mnewton_max_features(99) == 1, "the LDS budget (see above)");
static_assert(mnewton_max_features(100) == 0 && mnewton_max_features(1) == 0 && mnewton_max_features(0) == 0, "where nothing fits");

// Sparse x is expanded to a column-major dense copy by the driver (this mode's p is at most 98); the copy stays
// within the workspace bound of the Newton cross-validation (newton.hpp: 1 GiB).
constexpr size_t kMNewtonDenseCopyBytes = kNewtonCvWorkspaceBytes;

// ---- wide multinomial Newton mode (SGDNET_MODE_WMNEWTON): the same outer loop with the joint Hessian in global memory ----
// mnewton_wide_cd_kernel is ONE workgroup with newton_wide_cd_kernel's LDS layout over the Q = K (p + 1) coordinates:
//   the gradient g, U and diag H, in f64                               3 Q doubles
//   the list, its bits and the compaction's counts (wide_layout.hpp)    Q + ceil(Q / 32) + 32 words
// and H in global memory, leading dimension wide_leading_dim(Q), written by mnewton_wide_scale_kernel with diag H and q.
// In bytes: 24 Q + 4 Q + 4 ceil(Q / 32) + 128 <= 163 840:
//   Q = 5820:  162 960 + 728 + 128 = 163 816          Q = 5821:  162 988 + 728 + 128 = 163 844
// so K classes leave room for 5820 / K - 1 features: 2909 at K = 2, 1939 at K = 3, 581 at K = 10, 57 at K = 99.  K stays
// within 2 .. 99 as for mnewton: the class pair rides in blockIdx.z, and K (K + 1) / 2 = 4950 moment matrices is the most
// memory this mode should take.
constexpr int kWmnewtonLdsBytes = kWideLdsBytes;
constexpr int wmnewton_state_bytes(int Q) { return 24 * Q + wide_list_bytes(Q); }
constexpr int wmnewton_max_coordinates() {
  int Q = 1;
  while (wmnewton_state_bytes(Q + 1) <= kWmnewtonLdsBytes) ++Q;
  return Q;
}
constexpr int kWmnewtonMaxCoordinates = wmnewton_max_coordinates();
static_assert(kWmnewtonMaxCoordinates == 5820, "the LDS budget of the wide inner solve (see above)");
constexpr int kWmnewtonMaxClasses = 99;
constexpr int wmnewton_max_features(int K) {
  if (K < 2 || K > kWmnewtonMaxClasses) return 0;
  return kWmnewtonMaxCoordinates / K - 1;
}
static_assert(wmnewton_max_features(2) == 2909 && wmnewton_max_features(3) == 1939 && wmnewton_max_features(4) == 1454, "the LDS budget (see above)");
static_assert(wmnewton_max_features(5) == 1163 && wmnewton_max_features(10) == 581 && wmnewton_max_features(20) == 290, "the LDS budget (see above)");
static_assert(wmnewton_max_features(50) == 115 && wmnewton_max_features(99) == 57, "the LDS budget (see above)");
static_assert(wmnewton_max_features(100) == 0 && wmnewton_max_features(1) == 0 && wmnewton_max_features(0) == 0 && wmnewton_max_features(-3) == 0,
              "where nothing fits");

// The class-pair moments pass of the wide mode (mnewton_pair_tile_kernel, unchanged) launches tile pairs x class pairs
// workgroups per row chunk.  Its chunks follow wide_layout.hpp's wide_row_chunks with THAT product where the rule has
// the tile pairs: as many chunks as put about 1024 workgroups on the GPU, none shorter than 256 rows, ONE once a chunk
// alone has 1024 workgroups; the rows of a chunk rounded up to whole steps of tile_rows staged rows.
// (mnewton's dense_rows_per_chunk never takes fewer than 16 chunks: over 1 GB of partial tiles at ~50 000 workgroups.)
constexpr int64_t wmnewton_chunk_workgroups(int64_t ncols, int64_t K) { return wide_tile_pairs(ncols) * (K * (K + 1) / 2); }
constexpr int64_t wmnewton_row_chunks(int64_t n, int64_t ncols, int64_t K) {
  const int64_t wg = wmnewton_chunk_workgroups(ncols, K), cap = wg >= 1024 ? 1 : 1024 / wg, by_rows = (n + 255) / 256;
  return by_rows < 1 ? 1 : (by_rows < cap ? by_rows : cap);
}
constexpr int64_t wmnewton_rows_per_chunk(int64_t n, int64_t ncols, int64_t K, int64_t tile_rows) {
  return ((n + wmnewton_row_chunks(n, ncols, K) - 1) / wmnewton_row_chunks(n, ncols, K) + tile_rows - 1) / tile_rows * tile_rows;
}

// What the mode keeps in device memory beyond x and mu, at each K's feature limit (the largest p is the largest of each):
//   the joint matrix      wide_leading_dim(Q) Q doubles                     271.2 MB at K = 2 (Q = 5820)
//   the pair moments      K (K + 1) / 2 (p + 2)^2 doubles                   203.4 MB at K = 2 (3 x 2911^2)
//   the partial tiles     chunks x workgroups of a chunk x 256 doubles       125.8 MB at K = 90 (61 425 workgroups, one chunk);
//                         with several chunks there are at most 1024 workgroups in all: 2 MiB
constexpr int64_t kWmnewtonMatrixBytes = (int64_t)260 << 20, kWmnewtonMomentsBytes = (int64_t)194 << 20, kWmnewtonPartialBytes = (int64_t)120 << 20;
constexpr bool wmnewton_memory_fits() {
  for (int K = 2; K <= kWmnewtonMaxClasses; ++K) {
    const int64_t p = wmnewton_max_features(K), Q = K * (p + 1), nc = p + 2;
    if (Q > kWmnewtonMaxCoordinates || wide_leading_dim(Q) * Q * 8 > kWmnewtonMatrixBytes) return false;
    if ((int64_t)K * (K + 1) / 2 * nc * nc * 8 > kWmnewtonMomentsBytes) return false;
    // any n: the chunks are the cap's at most; fewer features only have fewer workgroups per chunk
    if (wmnewton_row_chunks((int64_t)1 << 40, nc, K) * wmnewton_chunk_workgroups(nc, K) * 256 * 8 > kWmnewtonPartialBytes) return false;
  }
  return true;
}
static_assert(wmnewton_memory_fits(), "the device memory of the wide mode at every K's limit (see above)");
static_assert(wmnewton_row_chunks((int64_t)1 << 40, 3, 2) * wmnewton_chunk_workgroups(3, 2) * 256 * 8 <= (int64_t)2 << 20 &&
              wmnewton_row_chunks((int64_t)1 << 40, 2911, 2) == 1, "1024 workgroups' tiles while there are chunks, one chunk at the limit");
// Sparse x is expanded to a column-major dense copy by the driver, as for mnewton; the copy stays within this many bytes.
constexpr size_t kWmnewtonDenseCopyBytes = (size_t)1 << 30;

struct MNewtonProblem : DirectProblem {         // x_dense only (sparse x: the driver's dense copy); max_iter: outer steps per lambda
  int K = 0;                           // classes
  const double* y = nullptr;           // n: class codes 0 .. K - 1
  bool fit_intercept = true;           // false: the intercepts stay at b0
  const double* b0 = nullptr;          // K: the null model's intercepts: where the path starts
};

struct MNewtonResult {
  std::vector<double> mean;            // p: the centres the deviations were taken from (0 where centre is false)
  std::vector<double> u;               // n_lambda x K (p + 1): per class the coefficients of the standardised problem, then the intercept at the centres
  std::vector<double> loss;            // n_lambda: mean multinomial loss at u
  std::vector<int32_t> steps;          // n_lambda: outer steps
  std::vector<int32_t> unconverged;    // n_lambda: all max_iter outer steps ran and tol was not met
  double passes = 0.0;                 // state passes over the whole path
  double sweeps = 0.0, halvings = 0.0; // (SGDNET_TRACE)
  float state_ms = 0.f, moments_ms = 0.f, cd_ms = 0.f;   // kernel times summed over the path (SGDNET_TRACE only: they cost a sync per step)
  float scale_ms = 0.f;                                  // wmnewton_run only: mnewton_wide_scale_kernel
};

// The Newton loop (mnewton.hip).  2 <= K and p <= mnewton_max_features(K) are the caller's business (plan_fit).
// timed: fill the *_ms fields.  width: lanes of the inner solve's workgroup (64 or 256), 0 = the rule of mnewton.hip
int mnewton_run(const MNewtonProblem& pb, bool timed, MNewtonResult* out, int width = 0);

// The same loop around the wide inner solve (mnewton.hip): 2 <= K <= 99 and p <= wmnewton_max_features(K) are the caller's
// business (plan_fit).  width: lanes of the inner solve's workgroup (256 or 1024), 0 = the rule of mnewton.hip
// (wmnewton_cd_width); both give the same bits.
int wmnewton_run(const MNewtonProblem& pb, bool timed, MNewtonResult* out, int width = 0);

// ---- cross-validation: every fold fit of every mix through the loop above in lock-step (mnewton.hip: mnewton_cv_run) ----
// Job (mix a, training set t) = a * n_sets + t is mnewton_run on the rows of its training set, as newton.hpp's
// newton_cv_run is newton_run: x and y come with the rows stably sorted by group, and with everything mnewton_run takes per
// problem per training set.  x is dense (sparse x: the driver's dense copy, as for a single fit).
//
// What a call keeps on the device, in doubles.  Per job: mu by LOCAL row (n_t K, a column per class: by global row the K
// columns of a job that trains on its fold would leave (G - 1) / G of them unused), the pair moments (K (K + 1) / 2 matrices
// of (p + 2)^2), the row chunks' partial tiles (chunks x tile pairs x K (K + 1) / 2 x 256, the chunks of the job with the
// most), the state pass's sums (1024), two iterates and the state-pass form of the candidate (3 Q), the record and the
// path (n_lambda Q).  Once: x and y (n (p + 1)).  Calls that need more than newton.hpp's kNewtonCvWorkspaceBytes are refused;
// so are those whose jobs (kNewtonCvMaxJobs) or jobs x class pairs do not fit a grid dimension.
constexpr int64_t kMNewtonCvMaxGridZ = 65535;
constexpr int kMNewtonCvStateMaxBlocks = 1024, kMNewtonCvRecordDoubles = 8;
// moments_device.hpp's dense_rows_per_chunk in plain constexpr (mnewton.hip checks the two against each other): at most
// max(16, min(256, 1024 / workgroups)) chunks, none shorter than 256 rows, whole steps of 64 staged rows
constexpr int64_t mnewton_cv_rows_per_chunk(int64_t n_t, int64_t workgroups) {
  const int64_t by_grid = 1024 / workgroups < 256 ? 1024 / workgroups : 256, cap = by_grid > 16 ? by_grid : 16;
  const int64_t by_rows = (n_t + 255) / 256, chunks = by_rows < cap ? by_rows : cap;
  return ((n_t + chunks - 1) / chunks + 63) / 64 * 64;
}
constexpr int64_t mnewton_cv_chunks(int64_t n_t, int64_t workgroups) {
  return (n_t + mnewton_cv_rows_per_chunk(n_t, workgroups) - 1) / mnewton_cv_rows_per_chunk(n_t, workgroups);
}
// n_t: the rows of each training set.  (In double: a call far beyond the bound must not wrap.)
constexpr double mnewton_cv_workspace_bytes(int64_t n, int64_t p, int K, const int64_t* n_t, int n_sets, int n_mix, int n_lambda) {
  const int64_t class_pairs = (int64_t)K * (K + 1) / 2, tile_pairs = wide_tile_pairs(p + 2), Q = (int64_t)K * (p + 1);
  int64_t max_chunks = 0;
  double rows = 0.0;
  for (int t = 0; t < n_sets; ++t) {
    const int64_t c = mnewton_cv_chunks(n_t[t], tile_pairs * class_pairs);
    max_chunks = c > max_chunks ? c : max_chunks;
    rows += (double)n_t[t];
  }
  const double per_job = (double)class_pairs * (double)((p + 2) * (p + 2)) + (double)max_chunks * (double)tile_pairs * (double)class_pairs * 256.0 +
                         (double)kMNewtonCvStateMaxBlocks + 3.0 * (double)Q + (double)kMNewtonCvRecordDoubles + (double)n_lambda * (double)Q;
  return 8.0 * ((double)n_mix * (rows * (double)K + (double)n_sets * per_job) + (double)n * (double)(p + 1));
}
constexpr int64_t kMNewtonCvFoldRows[10] = {30000, 30000, 30000, 30000, 30000, 30000, 30000, 30000, 30000, 30000};
// 50 jobs (5 mixes x 10 folds) of 30 000 rows each at K = 10 and its 18 features, 100 lambdas: about 455 MB
static_assert(mnewton_cv_workspace_bytes(300000, 18, 10, kMNewtonCvFoldRows, 10, 5, 100) <= (double)kNewtonCvWorkspaceBytes, "the workspace bound (see above)");
static_assert(mnewton_cv_chunks(1, 1) == 1 && mnewton_cv_chunks(335, 3) == 2 && mnewton_cv_chunks(903, 10) == 4 && mnewton_cv_chunks(100, 10) == 1 &&
              mnewton_cv_chunks((int64_t)1 << 30, 55 * 3) == 16 && mnewton_cv_chunks((int64_t)1 << 30, 1) == 256, "the row chunks (see above)");
static_assert(kNewtonCvMaxJobs <= kMNewtonCvMaxGridZ, "a job per workgroup of the inner solve's grid");

struct MNewtonCvProblem {
  int64_t n = 0, p = 0;
  int K = 0;                           // classes
  const double* x_dense = nullptr;     // column-major n x p, the rows sorted by group, in host memory
  const double* y = nullptr;           // n: class codes 0 .. K - 1, rows sorted as x's
  int n_sets = 0;                      // the groups; training set t is group t or everything else
  const int64_t* start = nullptr;      // n_sets + 1: the first row of each group
  bool train_on_rest = false;
  bool fit_intercept = true;
  const double* mean = nullptr;        // n_sets x p: the centres of training set t (its own column means; 0 where nothing is centred)
  const double* scale = nullptr;       // n_sets x p: the sd the driver standardises with over the training set (1 where it does not)
  const double* b0 = nullptr;          // n_sets x K: the null model's intercepts
  int device = 0;
  int n_mix = 0, n_lambda = 0;
  const double* l2 = nullptr;          // n_mix x n_lambda: regularization_path's alpha[l]
  const double* l1 = nullptr;          // n_mix x n_lambda: regularization_path's beta[l]
  const uint8_t* ridge = nullptr;      // n_mix: the ridge functor (no threshold)
  unsigned max_iter = 0;
  double tol = 0.0;
};

struct MNewtonCvResult {               // job-major
  std::vector<double> u;               // jobs x n_lambda x K (p + 1): as MNewtonResult::u, at the centres of the job's training set
  std::vector<double> loss;            // jobs x n_lambda
  std::vector<int32_t> unconverged;    // jobs x n_lambda
  std::vector<double> passes, steps, halvings;   // jobs: state passes, outer steps and halvings over the path
  double sweeps = 0.0;
  int rounds = 0;                      // rounds of the lock-step loop: launches shared by all jobs
  float moments_ms = 0.f, cd_ms = 0.f, state_ms = 0.f;   // (timed only)
};

// The lock-step loop.  The caller has checked the sizes, the feature limit, the job counts and the workspace.
int mnewton_cv_run(const MNewtonCvProblem& pb, bool timed, MNewtonCvResult* out);

// Diagnostics (include/sgdnet_hip.h: sgdnet_mnewton_probe): one outer step through the host steps mnewton_run takes, every
// output copied back.  pb: n, p, K, x_dense, y, centre, scale, device and n_lambda = 1; the rest is read from io.
int mnewton_probe(const MNewtonProblem& pb, sgdnet_mnewton_probe_io* io);
// sgdnet_wmnewton_probe: the same through the host steps wmnewton_run takes (io->width checked by the caller)
int wmnewton_probe(const MNewtonProblem& pb, sgdnet_wmnewton_probe_io* io);

}  // namespace sgdnet
