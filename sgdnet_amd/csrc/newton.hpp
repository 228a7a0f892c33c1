// Newton mode (SGDNET_MODE_NEWTON): what the plan, the driver and newton.hip share.
// No HIP type in here: fit_plan.hpp includes this file for the feature limit.
#pragma once

#include <stdint.h>

#include <vector>

#include "direct_problem.hpp"
#include "sgdnet_hip.h"
#include "wide_layout.hpp"

namespace sgdnet {

// The inner solve (newton.hip: newton_cd_kernel) is ONE wavefront that keeps, in f64, for one outer step over the
// P = p + 1 coordinates u = (w, b) -- the coefficients and the intercept --
//   the weighted Gram matrix H as a packed triangle     P (P + 1) / 2
//   u and the running gradient g = H (u - u0) - q        2 P
//   nothing else (u0 and q are read once, from memory; the sweep's reductions live in registers)
// in its LDS.  A workgroup of gfx950 may declare the CU's whole LDS, 160 KiB = 163 840 B = 20 480 doubles:
//   p = 198, P = 199:  19 900 + 398 = 20 298 <= 20 480          p = 199, P = 200:  20 100 + 400 = 20 500 > 20 480
constexpr int kNewtonLdsDoubles = 160 * 1024 / 8;
constexpr int newton_state_doubles(int p) { return (p + 1) * (p + 2) / 2 + 2 * (p + 1); }
constexpr int newton_max_features() {
  int p = 1;
  while (newton_state_doubles(p + 1) <= kNewtonLdsDoubles) ++p;
  return p;
}
constexpr int kNewtonMaxFeatures = newton_max_features();
static_assert(kNewtonMaxFeatures == 198, "the LDS budget of the inner solve (see above)");

// A candidate after which the penalised objective rose is moved half way back to the iterate it came from, at most this
// many times; the last halving is taken as it is (1 / 1024 of the step).
constexpr int kNewtonMaxHalvings = 10;
// "Rose": by more than this fraction of the objective.  Both objectives are sums of n rounded terms; near the optimum
// they agree to the last bits and the sign of their difference is noise, which must not halve a converging step.
constexpr double kNewtonObjectiveSlack = 1e-12;
// "All zero counts as converged", in floating point: at lambda_max the largest |q_j| EQUALS the threshold but for the
// rounding of two different sums, and what the threshold leaves of a coordinate is then a few units in the last place
// of q_j, different after every step: a relative change of order 1 in a number that means nothing.  A candidate
// whose every coordinate moves the linear predictor by no more than this, |u_j| sqrt(H_jj) (the v-weighted root mean
// square of u_j z_ij), is zero: 16 units in the last place of a linear predictor of size 1.
constexpr double kNewtonNegligible = 16 * 2.220446049250313e-16;
// Coordinate sweeps of one inner solve.  A solve cut short here is not lost: the next outer step starts from it, and a
// lambda is not done before an inner solve met the tolerance.
constexpr unsigned kNewtonMaxSweeps = 1000;

// ---- wide Newton mode (SGDNET_MODE_WNEWTON): the same outer loop with H in global memory ----
// newton_wide_cd_kernel is ONE workgroup that keeps, for one inner solve over the P = p + 1 coordinates, in its LDS
//   the gradient g, u and diag H, in f64                               3 P doubles
//   the list, its bits and the compaction's counts (wide_layout.hpp)    P + ceil(P / 32) + 32 words
// and H = M / n / (s s') in global memory, leading dimension wide_leading_dim(P), written by wide_scale_kernel with
// diag H and q.  In bytes: 24 P + 4 P + 4 ceil(P / 32) + 128 <= 163 840:
//   P = 5820:  162 960 + 728 + 128 = 163 816          P = 5821:  162 988 + 728 + 128 = 163 844
constexpr int kWnewtonLdsBytes = kWideLdsBytes;
constexpr int wnewton_state_bytes(int P) { return 24 * P + wide_list_bytes(P); }
constexpr int wnewton_max_features() {
  int p = 1;
  while (wnewton_state_bytes(p + 2) <= kWnewtonLdsBytes) ++p;
  return p;
}
constexpr int kWnewtonMaxFeatures = wnewton_max_features();
static_assert(kWnewtonMaxFeatures == 5819, "the LDS budget of the wide inner solve (see above)");
static_assert(kWnewtonMaxFeatures >= 4096, "include/sgdnet_hip.h promises at least 4096 features");

// The dense moments pass of the wide mode runs once per outer step over ncols = p + 2 columns (wide_layout.hpp:
// wide_row_chunks); its partial-tile buffer is 136 MB at the feature limit (364 tiles of 16 columns, 66 430 pairs).
// (newton mode's dense_rows_per_chunk never takes fewer than 16 chunks: 2.2 GB there.)
constexpr int64_t kWnewtonPartialBytes = (int64_t)160 << 20;
static_assert(wide_row_chunks(1 << 30, kWnewtonMaxFeatures + 2) == 1 &&
              wide_tile_pairs(kWnewtonMaxFeatures + 2) * 256 * 8 <= kWnewtonPartialBytes, "one chunk at the limit");
static_assert(wide_row_chunks(1 << 30, 3) * wide_tile_pairs(3) * 256 * 8 <= kWnewtonPartialBytes, "1024 workgroups' tiles at most");
// Sparse x is expanded to a column-major dense copy by the driver (the sparse pair kernel launches p (p + 2) workgroups per
// outer step); the copy stays within this many bytes.
constexpr size_t kWnewtonDenseCopyBytes = (size_t)1 << 30;

struct NewtonProblem : DirectProblem {          // max_iter: outer steps per lambda
  const double* y = nullptr;           // n: class codes 0 / 1
  bool fit_intercept = true;           // false: the last coordinate stays at b0
  double b0 = 0.0;                     // the null model's intercept: where the path starts
};

struct NewtonResult {
  std::vector<double> mean;            // p: the centres the deviations were taken from (0 where centre is false)
  std::vector<double> u;               // n_lambda x (p + 1): coefficients of the standardised problem, then the intercept at the centres
  std::vector<double> loss;            // n_lambda: mean binomial loss at u
  std::vector<int32_t> steps;          // n_lambda: outer steps
  std::vector<int32_t> unconverged;    // n_lambda: all max_iter outer steps ran and tol was not met
  double passes = 0.0;                 // state passes over the whole path
  double sweeps = 0.0, halvings = 0.0; // (SGDNET_TRACE)
  float state_ms = 0.f, moments_ms = 0.f, cd_ms = 0.f;   // kernel times summed over the path (SGDNET_TRACE only: they cost a sync per step)
  float scale_ms = 0.f;                                  // wnewton_run only: wide_scale_kernel
};

// The Newton loop (newton.hip).  p <= kNewtonMaxFeatures is the caller's business (plan_fit).  timed: fill the *_ms fields.
int newton_run(const NewtonProblem& pb, bool timed, NewtonResult* out);

// The same loop around the wide inner solve (newton.hip): dense x only, p <= kWnewtonMaxFeatures is the caller's business
// (plan_fit).  width: lanes of the inner solve's workgroup (256 or 1024), 0 = the rule of wide_layout.hpp (wide_cd_width);
// both give the same bits.
int wnewton_run(const NewtonProblem& pb, bool timed, NewtonResult* out, int width = 0);

// ---- cross-validation: every fold fit of every mix through the Newton loop in lock-step (newton.hip: newton_cv_run) ----
// Job (mix a, training set t) = a * n_sets + t is newton_run on the rows of its training set.  The caller hands x and y
// over with the rows stably sorted by group, so that a training set is the row range of its group
// [start[t], start[t + 1]) or the complement of it, and everything newton_run takes per problem per training set.
//
// What a call keeps on the device per job, in doubles: v and r (2 n: indexed by row, whichever rows the job trains on),
// the moments ((p + 2)^2) and, for dense x, the row chunks' partial tiles (chunks x tile pairs x 256; at most 16 x
// 91 x 256 at p = 198, 256 x 1 x 256 at p <= 14).  Calls whose jobs need more than this are refused.  1 GiB still holds
// 50 jobs (5 mixes x 10 folds) of 1.3 million rows at p <= 14, 50 jobs of 900 000 rows at p = 198, and a
// leave-one-out CV of 300 rows at p = 198 for 5 mixes (1500 jobs).
constexpr size_t kNewtonCvWorkspaceBytes = (size_t)1 << 30;
// the jobs ride in a grid dimension
constexpr int64_t kNewtonCvMaxJobs = 65535;

struct NewtonCvProblem {
  int64_t n = 0, p = 0;
  // x with its rows sorted by group: one of the two, in host memory
  const double* x_dense = nullptr;     // column-major n x p
  const int32_t* colptr = nullptr;     // p + 1; the rows of a column ascend
  const int32_t* rowidx = nullptr;
  const double* values = nullptr;
  const int32_t* cut = nullptr;        // sparse x: p x (n_sets + 1); cut[j][t] = the first entry of column j in a row >= start[t]
  const double* y = nullptr;           // n: class codes 0 / 1, rows sorted as x's
  int n_sets = 0;                      // the groups; training set t is group t or everything else
  const int64_t* start = nullptr;      // n_sets + 1: the first row of each group
  bool train_on_rest = false;
  bool centre = true, fit_intercept = true;
  const double* mean = nullptr;        // n_sets x p: the centres of training set t (its own column means; 0 where centre is false)
  const double* scale = nullptr;       // n_sets x p: the sd the driver standardises with over the training set (1 where it does not)
  const double* b0 = nullptr;          // n_sets: the null model's intercept
  int device = 0;
  int n_mix = 0, n_lambda = 0;
  const double* l2 = nullptr;          // n_mix x n_lambda: regularization_path's alpha[l]
  const double* l1 = nullptr;          // n_mix x n_lambda: regularization_path's beta[l]
  const uint8_t* ridge = nullptr;      // n_mix: the ridge functor (no threshold)
  unsigned max_iter = 0;
  double tol = 0.0;
};

struct NewtonCvResult {                // job-major
  std::vector<double> u;               // jobs x n_lambda x (p + 1): as NewtonResult::u, at the centres of the job's training set
  std::vector<double> loss;            // jobs x n_lambda
  std::vector<int32_t> unconverged;    // jobs x n_lambda
  std::vector<double> passes, steps, halvings;   // jobs: state passes, outer steps and halvings over the path
  double sweeps = 0.0;
  int rounds = 0;                      // rounds of the lock-step loop: launches shared by all jobs
  float moments_ms = 0.f, cd_ms = 0.f, state_ms = 0.f;   // (timed only)
  float scale_ms = 0.f;                                  // wnewton_cv_run only: newton_cv_wide_scale_kernel
};

// the device memory the jobs of a call need (see above); n_t: the rows of each training set
size_t newton_cv_workspace_bytes(int64_t n, int64_t p, bool sparse, const int64_t* n_t, int n_sets, int n_mix);

// The lock-step loop.  The caller has checked the sizes, the feature limit, the job count and the workspace.
int newton_cv_run(const NewtonCvProblem& pb, bool timed, NewtonCvResult* out);

// ---- the same for the wide mode (newton.hip: wnewton_cv_run) ----
// Job (mix a, training set t) = a * n_sets + t is wnewton_run on the rows of its training set: the lock-step loop above
// around the wide inner solve, dense x only, one workgroup -- one compute unit -- per job and round.  H depends on the
// iterate, so nothing is pooled across jobs: every job keeps its own, in doubles (P = p + 1, ld = wide_leading_dim(P)),
//   v and r                        2 n
//   the moments M                  (p + 2)^2
//   the row chunks' partial tiles  max_chunks x wide_tile_pairs(p + 2) x 256   (max_chunks: the most chunks of a job, each
//                                  job's being those wnewton_run takes for its n_t rows)
//   H, diag H and q                ld P + 2 P
//   the answers U                  n_lambda P
//   the small vectors              the state pass's sums (3 x 1024 + 2), the record, both iterates and the state-pass form (3 P)
// and once per call x and y (n p + n).  From 2000 features on a job is one chunk and about 2.5 (p + 2)^2 doubles.  With 100
// lambdas and 2000 rows: 50 jobs (5 mixes x 10 folds) take 1.07 GB at p = 1000 and 9.21 GB at p = 3000; at the limit
// p = 5819 a job is 0.68 GB (2.52 (p + 2)^2 doubles) and 25 jobs fit.  The bound is kWcovCvBytes's 16 GiB: the arithmetic
// gives no reason for another -- it is an eighteenth of the card's 288 GB, and it holds the 50-job CV up to 4110 features.
constexpr size_t kWnewtonCvBytes = (size_t)16 << 30;
constexpr int kWnewtonCvTileRows = 64, kWnewtonCvStateMaxBlocks = 1024, kWnewtonCvRecordDoubles = 8;     // (newton.hip asserts them)
// the row chunks wnewton_run takes for n rows
constexpr int64_t wnewton_row_chunks(int64_t n, int64_t p) {
  return (n + wide_rows_per_chunk(n, p + 2, kWnewtonCvTileRows) - 1) / wide_rows_per_chunk(n, p + 2, kWnewtonCvTileRows);
}
constexpr size_t wnewton_cv_bytes(int64_t jobs, int64_t n, int64_t p, int64_t n_lambda, int64_t max_chunks) {
  return sizeof(double) * ((size_t)jobs * (2 * (size_t)n + (size_t)(p + 2) * (size_t)(p + 2) +
                                           (size_t)max_chunks * (size_t)wide_tile_pairs(p + 2) * 256 +
                                           (size_t)wide_leading_dim(p + 1) * (size_t)(p + 1) + 2 * (size_t)(p + 1) +
                                           (size_t)n_lambda * (size_t)(p + 1) + 3 * (size_t)kWnewtonCvStateMaxBlocks + 2 +
                                           (size_t)kWnewtonCvRecordDoubles + 3 * (size_t)(p + 1)) +
                           (size_t)n * (size_t)p + (size_t)n);
}
static_assert(wnewton_row_chunks(2000, 1000) == 1 && wnewton_row_chunks(2000, 3000) == 1, "one chunk from 1024 tile pairs on");
static_assert(wnewton_cv_bytes(50, 2000, 1000, 100, 1) / 10000000 == 107 && wnewton_cv_bytes(50, 2000, 3000, 100, 1) / 10000000 == 921,
              "the examples above");
static_assert((wnewton_cv_bytes(2, 2000, kWnewtonMaxFeatures, 100, 1) - wnewton_cv_bytes(1, 2000, kWnewtonMaxFeatures, 100, 1)) / 10000000 == 68,
              "the examples above");
static_assert(wnewton_cv_bytes(25, 2000, kWnewtonMaxFeatures, 100, 1) <= kWnewtonCvBytes &&
              wnewton_cv_bytes(26, 2000, kWnewtonMaxFeatures, 100, 1) > kWnewtonCvBytes, "the examples above");
static_assert(wnewton_cv_bytes(50, 2000, 4110, 100, 1) <= kWnewtonCvBytes && wnewton_cv_bytes(50, 2000, 4111, 100, 1) > kWnewtonCvBytes,
              "the examples above");

// the device memory the jobs of a call need (see above); n_t: the rows of each training set
size_t wnewton_cv_workspace_bytes(int64_t n, int64_t p, const int64_t* n_t, int n_sets, int n_mix, int n_lambda);

// The lock-step loop around the wide inner solve: pb as newton_cv_run takes it, dense x only.  width as wnewton_run's.  The
// caller has checked the sizes, the feature limit, the job count, the width and the workspace.
int wnewton_cv_run(const NewtonCvProblem& pb, bool timed, NewtonCvResult* out, int width = 0);

// Diagnostics (include/sgdnet_hip.h: sgdnet_newton_probe_*): one outer step through the host steps newton_run takes, every
// output copied back.  pb: x, y, centre, scale, device and n_lambda = 1; the rest comes from io.  The caller has checked both.
int newton_probe(const NewtonProblem& pb, sgdnet_newton_probe* io);
// sgdnet_wnewton_probe: the same through the host steps wnewton_run takes (dense x; io->width checked by the caller)
int wnewton_probe(const NewtonProblem& pb, sgdnet_wnewton_probe_io* io);

}  // namespace sgdnet
