// Covariance mode (SGDNET_MODE_COVARIANCE): what the plan, the driver and covariance.hip share.
// No HIP type in here: fit_plan.hpp includes this file for the feature limit.
#pragma once

#include <stdint.h>

#include <vector>

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

struct CovarianceProblem {
  int64_t n = 0, p = 0;
  // x as the fit entry points receive it: one of the two, in host memory
  const double* x_dense = nullptr;     // column-major n x p
  const int32_t* colptr = nullptr;     // dgCMatrix slots; row indices ascending within a column
  const int32_t* rowidx = nullptr;
  const double* values = nullptr;
  const double* y = nullptr;           // n: the response as the solvers see it (centred and scaled by the driver)
  bool centre = true;                  // deviations from the column means (false: from 0 -- no intercept, no standardisation)
  const double* scale = nullptr;       // p: the sd the driver standardises feature j with (1 where it does not)
  int device = 0;
  // the path, in the driver's units (regularization_path): l2 strength alpha[l], l1 strength beta[l]
  int n_lambda = 0;
  const double* alpha = nullptr;
  const double* beta = nullptr;
  bool ridge = false;                  // the ridge functor: no threshold
  unsigned max_iter = 0;               // coordinate sweeps per lambda
  double tol = 0.0;
};

struct CovarianceResult {
  std::vector<double> mean;            // p: the centres the deviations were taken from (0 where centre is false)
  std::vector<double> c;               // p: c~_j = sum_i x~_ij y~_i / n
  std::vector<double> w, g;            // n_lambda x p: coefficients and gradient S w - c~ of the standardised problem
  std::vector<int32_t> sweeps;         // n_lambda
  std::vector<int32_t> unconverged;    // n_lambda: all max_iter sweeps ran and tol was not met
  float moments_ms = 0.f, path_ms = 0.f;   // kernel times (SGDNET_TRACE)
};

// Moments pass + path kernel (covariance.hip).  p <= kCovMaxFeatures is the caller's business (plan_fit).
int covariance_run(const CovarianceProblem& pb, CovarianceResult* out);

}  // namespace sgdnet
