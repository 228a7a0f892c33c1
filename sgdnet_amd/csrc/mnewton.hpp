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
};

// The Newton loop (mnewton.hip).  2 <= K and p <= mnewton_max_features(K) are the caller's business (plan_fit).
// timed: fill the *_ms fields.  width: lanes of the inner solve's workgroup (64 or 256), 0 = the rule of mnewton.hip
int mnewton_run(const MNewtonProblem& pb, bool timed, MNewtonResult* out, int width = 0);

// Diagnostics (include/sgdnet_hip.h: sgdnet_mnewton_probe): one outer step through the host steps mnewton_run takes, every
// output copied back.  pb: n, p, K, x_dense, y, centre, scale, device and n_lambda = 1; the rest is read from io.
int mnewton_probe(const MNewtonProblem& pb, sgdnet_mnewton_probe_io* io);

}  // namespace sgdnet
