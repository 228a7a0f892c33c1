// Covariance mode (SGDNET_MODE_COVARIANCE): what the plan, the driver and covariance.hip share.
// No HIP type in here: fit_plan.hpp includes this file for the feature limit.
#pragma once

#include <stdint.h>

#include <map>
#include <string>
#include <vector>

#include "direct_problem.hpp"
#include "group_rows.hpp"
#include "wide_layout.hpp"

namespace sgdnet {

// The path kernel (covariance.hip: cov_path_kernel) is ONE workgroup that keeps, in f64, for the whole lambda path
//   the scaled Gram matrix S as a packed triangle      p (p + 1) / 2
//   c~ = X~'y~ / n, the coefficients w, the gradient    3 p
//   nothing else (the sweep's reductions live in registers: every lane computes the same scalars)
// in its LDS.  A workgroup of gfx950 may declare the CU's whole LDS, 160 KiB = 163 840 B = 20 480 doubles:
//   p = 198:  19 701 + 594 = 20 295 <= 20 480          p = 199:  19 900 + 597 = 20 497 > 20 480
constexpr int kCovLdsDoubles = 160 * 1024 / 8;
constexpr int cov_state_doubles(int p) { return p * (p + 1) / 2 + 3 * p; }
constexpr int cov_max_features() {
  int p = 1;
  while (cov_state_doubles(p + 1) <= kCovLdsDoubles) ++p;
  return p;
}
constexpr int kCovMaxFeatures = cov_max_features();
static_assert(kCovMaxFeatures == 198, "the LDS budget of the path kernel (see above)");
static_assert(kCovMaxFeatures >= 64, "include/sgdnet_hip.h promises at least 64 features");

// Diagnostics (include/sgdnet_hip.h: sgdnet_covariance_path_probe, sgdnet_cv_covariance_probe).  A run that is handed a tap
// appends, behind the stages that wrote them and before the path kernel is launched, device-to-host copies of what those
// stages left, under the names the header lists; and, once the path kernel has been enqueued, of the four buffers it
// wrote (W, G, sweeps, unconverged: the device buffers themselves, in the kernel's layout), with the tol and max_iter the
// kernel was handed.  A fit passes null: not a launch, a grid or an argument differs, with a tap or without.
struct CovTap {
  std::map<std::string, std::vector<double>> f64;
  std::map<std::string, std::vector<int32_t>> i32;
};

struct CovarianceProblem : DirectProblem {      // max_iter: coordinate sweeps per lambda
  const double* y = nullptr;           // n: the response as the solvers see it (centred and scaled by the driver)
};

struct CovarianceResult {
  std::vector<double> mean;            // p: the centres the deviations were taken from (0 where centre is false)
  std::vector<double> c;               // p: c~_j = sum_i x~_ij y~_i / n
  std::vector<double> w, g;            // n_lambda x p: coefficients and gradient S w - c~ of the standardised problem
  std::vector<int32_t> sweeps;         // n_lambda
  std::vector<int32_t> unconverged;    // n_lambda: all max_iter sweeps ran and tol was not met
  float moments_ms = 0.f, path_ms = 0.f;   // kernel times (SGDNET_TRACE)
  float scale_ms = 0.f;                    // wcovariance_run only: wide_scale_kernel
};

// Moments pass + path kernel (covariance.hip).  p <= kCovMaxFeatures is the caller's business (plan_fit).
int covariance_run(const CovarianceProblem& pb, CovarianceResult* out, CovTap* tap = nullptr);

// ---- wide covariance mode (SGDNET_MODE_WCOVARIANCE): the same path with S in global memory ----
// cov_wide_path_kernel is ONE workgroup that keeps, for the whole lambda path, in its LDS
//   the gradient g, c~, the coefficients w and diag S, in f64        4 p doubles
//   the list, its bits and the compaction's counts (wide_layout.hpp)  p + ceil(p / 32) + 32 words
// and S = C / (n sd sd') in global memory, leading dimension wide_leading_dim(p), written by wide_scale_kernel.
// In bytes: 32 p + 4 p + 4 ceil(p / 32) + 128 <= 163 840:
//   p = 4531:  163 116 + 568 + 128 = 163 812          p = 4532:  163 152 + 568 + 128 = 163 848
constexpr int kCovLdsBytes = kWideLdsBytes;
constexpr int wcov_state_bytes(int p) { return 32 * p + wide_list_bytes(p); }
constexpr int wcov_max_features() {
  int p = 1;
  while (wcov_state_bytes(p + 1) <= kCovLdsBytes) ++p;
  return p;
}
constexpr int kWcovMaxFeatures = wcov_max_features();
static_assert(kWcovMaxFeatures == 4531, "the LDS budget of the wide path kernel (see above)");
static_assert(kWcovMaxFeatures >= 4096, "include/sgdnet_hip.h promises at least 4096 features");

// The dense moments pass of the wide mode runs over ncols = p + 1 columns (wide_layout.hpp: wide_row_chunks); its
// partial-tile buffer is 82.9 MB at the feature limit (284 tiles of 16 columns, 40 470 pairs).
constexpr int64_t kWcovPartialBytes = (int64_t)96 << 20;
static_assert(wide_row_chunks(1 << 30, kWcovMaxFeatures + 1) == 1 && wide_tile_pairs(kWcovMaxFeatures + 1) * 256 * 8 <= kWcovPartialBytes,
              "one chunk at the limit");
static_assert(wide_row_chunks(1 << 30, 2) * wide_tile_pairs(2) * 256 * 8 <= kWcovPartialBytes, "1024 workgroups' tiles at most");

// Moments pass + wide_scale_kernel + cov_wide_path_kernel (covariance.hip).  p <= kWcovMaxFeatures is the caller's
// business (plan_fit).  width: lanes of the path kernel's workgroup (256 or 1024), 0 = the rule of wide_layout.hpp
// (wide_cd_width); both give the same bits.
int wcovariance_run(const CovarianceProblem& pb, CovarianceResult* out, int width = 0, CovTap* tap = nullptr);

// ---- several responses (SGDNET_MODE_MCOVARIANCE): the mgaussian group-lasso path ----
// cov_group_path_kernel keeps the same packed triangle S (one Gram matrix serves all K responses) and c~, w and the
// gradient as p x K each, entry (j, r) at j K + r:
//   p (p + 1) / 2 + 3 p K doubles
// One response would give the 198 features above; K = 2 gives 195 (19 110 + 1 170 = 20 280), K = 10 gives 174
// (15 225 + 5 220 = 20 445), K = 96 gives 63 (2 016 + 18 144 = 20 160).  Nothing fits from K = 6 827 on (a single
// feature needs 1 + 3 K doubles).
constexpr int64_t mcov_state_doubles(int64_t p, int64_t K) { return p * (p + 1) / 2 + 3 * p * K; }
constexpr int mcov_max_features(int K) {
  if (K < 1 || mcov_state_doubles(1, K) > kCovLdsDoubles) return 0;
  int p = 1;
  while (mcov_state_doubles(p + 1, K) <= kCovLdsDoubles) ++p;
  return p;
}
static_assert(mcov_max_features(1) == kCovMaxFeatures, "one response: the budget of cov_path_kernel");
static_assert(mcov_max_features(2) == 195 && mcov_max_features(3) == 193 && mcov_max_features(5) == 187, "the LDS budget (see above)");
static_assert(mcov_max_features(10) == 174 && mcov_max_features(16) == 159 && mcov_max_features(32) == 127, "the LDS budget (see above)");
static_assert(mcov_max_features(64) == 86 && mcov_max_features(95) == 64 && mcov_max_features(96) == 63, "the LDS budget (see above)");
static_assert(mcov_max_features(0) == 0 && mcov_max_features(6826) == 1 && mcov_max_features(6827) == 0, "where nothing fits");

struct McovarianceProblem : DirectProblem {     // beta: the group threshold; max_iter: block sweeps per lambda
  int K = 0;                           // responses
  const double* y = nullptr;           // n x K, column-major: the responses less the null model's intercepts
};

struct McovarianceResult {
  std::vector<double> mean;            // p
  std::vector<double> c;               // p x K, entry (j, r) at j K + r: c~_jr = sum_i x~_ij y~_ir / n
  std::vector<double> w, g;            // n_lambda x p x K
  std::vector<int32_t> sweeps, unconverged;   // n_lambda
  float moments_ms = 0.f, path_ms = 0.f;
  float scale_ms = 0.f;                // wmcovariance_run only: cov_wide_group_scale_kernel
};

// Moments pass + cov_group_path_kernel (covariance.hip).  p <= mcov_max_features(K) is the caller's business (plan_fit).
// width: lanes of the path kernel's workgroup (64 or 256), 0 = the rule of covariance.hip (mcov_path_width)
int mcovariance_run(const McovarianceProblem& pb, McovarianceResult* out, int width = 0, CovTap* tap = nullptr);

// ---- wide multi-response mode (SGDNET_MODE_WMCOVARIANCE): the mgaussian path with S in global memory ----
// cov_wide_group_path_kernel is ONE workgroup that keeps, for the whole lambda path, in its LDS
//   the gradient g and the coefficients w, response-major: K vectors each, a vector
//   padded to the even length pe = p + (p & 1) so that the 16-byte slots of the column
//   move stay aligned in every response                                               2 K pe doubles
//   diag S                                                                            p doubles
//   the new coefficients of the block that moves (scratch)                            K doubles
//   the list, its bits and the compaction's counts (wide_layout.hpp)                  p + ceil(p / 32) + 32 words
// and S in global memory as cov_wide_path_kernel has it.  c~ = X~'Y~ / n stays in global memory too: it is read once per
// lambda, when g is rebuilt, and by nothing in the sweep (in LDS it would cost 8 K p more bytes and the limit at K = 2 would be about 2700 features).
// In bytes: 16 K pe + 8 p + 8 K + 4 p + 4 ceil(p / 32) + 128 <= 163 840:
//   K = 2:   p = 3709: 163 836      p = 3710: 163 848          K = 10:  p = 950: 163 728      p = 951: 164 060
//   K = 3:   p = 2722: 163 816      p = 2723: 163 924          K = 96:  p = 104: 161 904      p = 105: 164 988
// One feature alone needs 40 K + 144 bytes (pe = 2): nothing fits from K = 4093 on.
// The moments pass runs over p + K columns, and it stays within the column count and the partial-tile buffer that
// wcovariance_run already runs (kWcovPartialBytes): p + K <= kWcovMaxFeatures + 1.  That, not the LDS, is the limit of one
// response (4531; the LDS would hold 5824), which SGDNET_MODE_WCOVARIANCE serves anyway.
constexpr int64_t wmcov_state_bytes(int64_t p, int64_t K) {
  return 16 * K * (p + (p & 1)) + 8 * p + 8 * K + 4 * p + 4 * ((p + 31) / 32) + 4 * kWideScanWords;
}
constexpr bool wmcov_fits(int64_t p, int64_t K) { return wmcov_state_bytes(p, K) <= kWideLdsBytes && p + K <= kWcovMaxFeatures + 1; }
constexpr int wmcov_max_features(int K) {
  if (K < 1 || !wmcov_fits(1, K)) return 0;
  int p = 1;
  while (wmcov_fits(p + 1, K)) ++p;
  return p;
}
static_assert(wmcov_state_bytes(4531, 1) - 8 * 4531 - 16 * 4532 - 8 == wide_list_bytes(4531), "the list's share is wide_layout.hpp's");
static_assert(wmcov_max_features(1) == kWcovMaxFeatures, "one response: the column count of the moments pass");
static_assert(wmcov_max_features(2) == 3709 && wmcov_max_features(3) == 2722, "the LDS budget (see above)");
static_assert(wmcov_max_features(10) == 950 && wmcov_max_features(96) == 104, "the LDS budget (see above)");
static_assert(wmcov_max_features(0) == 0 && wmcov_max_features(-1) == 0 && wmcov_max_features(4092) == 2 && wmcov_max_features(4093) == 0 &&
              wmcov_max_features(2147483647) == 0, "where nothing fits");
static_assert(wmcov_max_features(2) >= 2048 && wmcov_max_features(10) >= 512, "include/sgdnet_hip.h promises these");
// the moments pass of every accepted shape: no more columns than wcovariance_run's at its limit, so one chunk of rows
// once the tile pairs reach 1024 and the same bound on the partial tiles
static_assert(wmcov_max_features(1) + 1 <= kWcovMaxFeatures + 1 && wmcov_max_features(2) + 2 <= kWcovMaxFeatures + 1 &&
              wmcov_max_features(4092) + 4092 <= kWcovMaxFeatures + 1, "p + K within the columns of wcovariance_run's moments pass");

// Moments pass + cov_wide_group_scale_kernel + cov_wide_group_path_kernel (covariance.hip).  p <= wmcov_max_features(K) is
// the caller's business (plan_fit).  width: lanes of the path kernel's workgroup (256 or 1024), 0 = the rule of
// covariance.hip (wmcov_path_width: 256 up to 1024 features); both give the same bits.
int wmcovariance_run(const McovarianceProblem& pb, McovarianceResult* out, int width = 0, CovTap* tap = nullptr);

// ---- cross-validation: every (training set, elastic-net mix) path of one x in one launch ----
// Rows carry a group id fold[i] in [0, G).  One pass leaves, per group and about ONE centre a (the whole-data column
// means, or 0 where centre is false; mean(y) for the response), the (p + 2) x (p + 2) moment matrix of the augmented
// rows [x - a | y - a_y | 1]: the cross-products C^g, the sums of deviations s^g (last column) and n_g (last entry).
// A training set T is one group or all groups but one; cov_assemble_kernel pools its groups and re-centres to T's own
// means into what cov_path_kernel reads.  A job is (mix, T): job = mix_index * G + T.
//
// The budget of the group moments: G (p + 2)^2 doubles.  64 MiB holds nfolds = n for every n up to 209 at p = 198 and
// up to 524 288 at p = 2; a 10-fold CV at p = 198 takes 3.2 MB of it.
constexpr size_t kCovGroupMomentBytes = (size_t)64 << 20;
constexpr int kCovMaxRowChunks = 65535;   // the dense moments pass puts its row chunks (at least one per group) on gridDim.y
// The chunks are group_rows.hpp's: group_row_chunks(count, G, cov_rows_per_chunk(n, p + K + 1, wide)) predicts what the
// runs below launch from group_rows() at the same rows per chunk (one response: K = 1).

struct CovarianceCvProblem {
  int64_t n = 0, p = 0;
  const double* x_dense = nullptr;     // as CovarianceProblem: x and y in host memory, as they came
  const int32_t* colptr = nullptr;
  const int32_t* rowidx = nullptr;
  const double* values = nullptr;
  const double* y = nullptr;           // n: the response as it came (NOT preprocessed: every training set has its own centre)
  const int32_t* fold = nullptr;       // n: group ids in [0, n_groups), no group empty (the caller's business)
  int n_groups = 0;
  bool train_on_rest = false;          // T = all groups but one (false: T = one group)
  bool centre = true, standardize = true;
  int device = 0;
  int n_mix = 0, n_lambda = 0;
  const double* mix = nullptr;         // n_mix
  const double* lambda = nullptr;      // n_mix x n_lambda, a row per mix
  unsigned max_iter = 0;
  double tol = 0.0;
};

struct CovarianceCvResult {
  // per training set T (n_groups of them)
  std::vector<double> n_train;         // G
  std::vector<double> mean;            // G x (p + 1): the means of x (0 where centre is false) and of y over T
  std::vector<double> scale;           // G x p: the sd feature j is standardised with (1 without standardize)
  std::vector<double> y_scale, yy;     // G: sd of y over T (0 -> 1); y~'y~ of the preprocessed response
  // per job
  std::vector<double> c;               // jobs x p
  std::vector<double> w, g;            // jobs x n_lambda x p
  std::vector<int32_t> sweeps, unconverged;   // jobs x n_lambda
  float moments_ms = 0.f, assemble_ms = 0.f, path_ms = 0.f;
};

// Group moments + assembly + path kernel over the jobs.  p <= kCovMaxFeatures, the budget above and valid fold ids are
// the caller's business (driver_direct.cpp: fit_cv_covariance).
int covariance_cv_run(const CovarianceCvProblem& pb, CovarianceCvResult* out, CovTap* tap = nullptr);

// ---- the same in wide covariance mode (SGDNET_MODE_WCOVARIANCE): beyond kCovMaxFeatures features ----
// The same group moments (over p + 2 columns; dense x: row chunks by wide_rows_per_chunk, cut at the groups' ends), pooled
// and re-centred per training set straight into the scaled Gram matrices S_T in global memory (leading dimension
// wide_leading_dim(p), set stride ld p), and cov_wide_path_kernel's path over the jobs: one workgroup, one CU, per job.
//
// The budget, in doubles: the group moments G (p + 2)^2, their total (p + 2)^2, the dense partial tiles chunks x
// wide_tile_pairs(p + 2) x 256 (none for sparse x) and the scaled matrices G ld p -- x and the per-job outputs are not
// counted.  At the feature limit a group is 164.4 + 82.9 + 164.7 MB (one chunk per group from 1024 tile pairs on):
// a 10-fold CV takes 4.28 GB and a 20-fold 8.40 GB of the 16 GiB; at p = 1000 a group is 20.2 MB and 849 groups fit.
constexpr size_t kWcovCvBytes = (size_t)16 << 30;
constexpr size_t wcov_cv_bytes(int64_t G, int64_t p, int64_t chunks) {
  return sizeof(double) * ((size_t)(G + 1) * (size_t)(p + 2) * (size_t)(p + 2) + (size_t)chunks * (size_t)wide_tile_pairs(p + 2) * 256 +
                           (size_t)G * (size_t)wide_leading_dim(p) * (size_t)p);
}
static_assert(wcov_cv_bytes(10, kWcovMaxFeatures, 10) <= kWcovCvBytes, "a 10-fold CV at the feature limit fits");
static_assert(wcov_cv_bytes(10, kWcovMaxFeatures, 10) / 10000000 == 428 && wcov_cv_bytes(20, kWcovMaxFeatures, 20) / 10000000 == 840,
              "the examples above");
static_assert(wcov_cv_bytes(849, 1000, 849) <= kWcovCvBytes && wcov_cv_bytes(850, 1000, 850) > kWcovCvBytes, "the examples above");

// Group moments + stats and assembly + wide path kernel over the jobs.  p <= kWcovMaxFeatures, the budget above, at most
// kCovMaxRowChunks row chunks (dense) or groups (sparse) and valid fold ids are the caller's business (driver_direct.cpp:
// fit_cv_wcovariance).  width as in wcovariance_run.
int wcovariance_cv_run(const CovarianceCvProblem& pb, CovarianceCvResult* out, int width = 0, CovTap* tap = nullptr);

// ---- the same for K responses (SGDNET_MODE_MCOVARIANCE) ----
// The augmented rows are [x - a | y_1 - a_y1 .. y_K - a_yK | 1]: per group a (p + K + 1) x (p + K + 1) moment matrix, the
// response-by-response block included (a training set's y~'y~ and null deviance come from its diagonal).
// mcov_assemble_kernel re-centres every response to its own mean over T -- the null model's intercept, subtracted before
// anything is multiplied because the moments are of deviations about a centre of the order of that mean -- and divides it
// by its sd over T only with standardize_response; the penalties are (1 - mix) lambda and mix lambda (mgaussian: y_scale
// = 1).  A job is (mix, T) as above and runs cov_group_path_kernel, one workgroup and one CU's LDS each.
//
// The budget: G (p + K + 1)^2 doubles within kCovGroupMomentBytes, so p + K + 1 <= 2896 whatever G is and the assembly's
// staging (2 (p + K) doubles and p + K ints of LDS) stays below 64 KiB.  At K = 96, p = 63 a 10-fold CV takes 2.0 MB of it.
constexpr size_t mcov_group_moment_bytes(int64_t G, int64_t p, int64_t K) {
  return (size_t)G * (size_t)(p + K + 1) * (size_t)(p + K + 1) * sizeof(double);
}

struct McovarianceCvProblem {
  int64_t n = 0, p = 0;
  int K = 0;                           // responses
  const double* x_dense = nullptr;     // as CovarianceCvProblem
  const int32_t* colptr = nullptr;
  const int32_t* rowidx = nullptr;
  const double* values = nullptr;
  const double* y = nullptr;           // n x K, column-major: the responses as they came
  const int32_t* fold = nullptr;       // n: group ids in [0, n_groups), no group empty (the caller's business)
  int n_groups = 0;
  bool train_on_rest = false;
  bool centre = true, standardize = true, standardize_response = false;
  int device = 0;
  int n_mix = 0, n_lambda = 0;
  const double* mix = nullptr;         // n_mix
  const double* lambda = nullptr;      // n_mix x n_lambda, a row per mix
  unsigned max_iter = 0;
  double tol = 0.0;
  int width = 0;                       // lanes of the path kernel's workgroup (64 or 256), 0 = mcov_path_width; the same bits
};

struct McovarianceCvResult {
  // per training set T (n_groups of them)
  std::vector<double> n_train;         // G
  std::vector<double> mean;            // G x (p + K): the means of x over T (0 where centre is false), then the null model's
                                       // intercepts of the responses as the fit sees them (mean_T(y_r); 0 once standardised)
  std::vector<double> scale;           // G x p
  std::vector<double> yy, nulldev;     // G: sum_r y~_r'y~_r of the preprocessed responses; the null deviance of y[T] as it came
  // per job
  std::vector<double> c;               // jobs x p x K, entry (j, r) at j K + r
  std::vector<double> w, g;            // jobs x n_lambda x p x K
  std::vector<int32_t> sweeps, unconverged;   // jobs x n_lambda
  float moments_ms = 0.f, assemble_ms = 0.f, path_ms = 0.f;
};

// Group moments + assembly + path kernel over the jobs.  p <= mcov_max_features(K), the budget above, at most
// kCovMaxRowChunks row chunks (dense) or groups (sparse) and valid fold ids are the caller's business
// (driver_direct.cpp: fit_cv_mcovariance).
int mcovariance_cv_run(const McovarianceCvProblem& pb, McovarianceCvResult* out, CovTap* tap = nullptr);

// ---- the same in wide multi-response mode (SGDNET_MODE_WMCOVARIANCE): beyond mcov_max_features(K) features ----
// The same group moments over Pa = p + K + 1 columns (dense x: row chunks by wide_rows_per_chunk, cut at the groups' ends),
// pooled and re-centred per training set straight into the scaled Gram matrices S_T (leading dimension wide_leading_dim(p),
// set stride ld p) and c~_T (p x K, entry (j, r) at j K + r) in global memory, and cov_wide_group_path_kernel's path over
// the jobs: one workgroup, one CU, per job.
//
// The budget, in doubles: the group moments and their total (G + 1) Pa^2, the dense partial tiles chunks x
// wide_tile_pairs(Pa) x 256 (none for sparse x), the scaled matrices G ld p and c~ G p K -- x and the per-job outputs are
// not counted.  It is held within kWcovCvBytes.  At the limit of K = 2 (3709 features) a 10-fold CV takes 2.87 GB and a
// 20-fold 5.63 GB; at the limit of K = 10 (950) a 10-fold takes 0.19 GB; at p = 1000, K = 2 a group is 20.3 MB and 847
// groups fit.
constexpr size_t wmcov_cv_bytes(int64_t G, int64_t p, int64_t K, int64_t chunks) {
  return sizeof(double) * ((size_t)(G + 1) * (size_t)(p + K + 1) * (size_t)(p + K + 1) + (size_t)chunks * (size_t)wide_tile_pairs(p + K + 1) * 256 +
                           (size_t)G * (size_t)wide_leading_dim(p) * (size_t)p + (size_t)G * (size_t)p * (size_t)K);
}
static_assert(wmcov_cv_bytes(10, wmcov_max_features(2), 2, 10) <= kWcovCvBytes && wmcov_cv_bytes(10, wmcov_max_features(10), 10, 10) <= kWcovCvBytes,
              "a 10-fold CV at the feature limits of K = 2 and K = 10 fits");
static_assert(wmcov_cv_bytes(10, 3709, 2, 10) / 10000000 == 286 && wmcov_cv_bytes(20, 3709, 2, 20) / 10000000 == 562 &&
              wmcov_cv_bytes(10, 950, 10, 10) / 10000000 == 19, "the examples above");
static_assert(wmcov_cv_bytes(847, 1000, 2, 847) <= kWcovCvBytes && wmcov_cv_bytes(848, 1000, 2, 848) > kWcovCvBytes, "the examples above");
// wmcov_fits keeps p + K <= kWcovMaxFeatures + 1, so Pa <= 4533 and Pa^2 = 20 548 089 at most: cov_total_kernel's int
static_assert((int64_t)(kWcovMaxFeatures + 2) * (kWcovMaxFeatures + 2) <= 2147483647, "Pa^2 fits cov_total_kernel's int");

// Group moments + stats and assembly + wide group path kernel over the jobs.  p <= wmcov_max_features(K), the budget above,
// at most kCovMaxRowChunks row chunks (dense) or groups (sparse) and valid fold ids are the caller's business
// (driver_direct.cpp: fit_cv_mcovariance, wide).  width: lanes of the path kernel's workgroup (256 or 1024), 0 = the rule
// of covariance.hip (wmcov_path_width); both give the same bits.  pb.width is not read.
int wmcovariance_cv_run(const McovarianceCvProblem& pb, McovarianceCvResult* out, int width = 0, CovTap* tap = nullptr);

}  // namespace sgdnet
