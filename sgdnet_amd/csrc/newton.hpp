// Newton mode (SGDNET_MODE_NEWTON): what the plan, the driver and newton.hip share.
// No HIP type in here: fit_plan.hpp includes this file for the feature limit.
#pragma once

#include <stdint.h>

#include <vector>

#include "sgdnet_hip.h"

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

struct NewtonProblem {
  int64_t n = 0, p = 0;
  // x as the fit entry points receive it: one of the two, in host memory
  const double* x_dense = nullptr;     // column-major n x p
  const int32_t* colptr = nullptr;     // dgCMatrix slots
  const int32_t* rowidx = nullptr;
  const double* values = nullptr;
  const double* y = nullptr;           // n: class codes 0 / 1
  bool centre = true;                  // deviations from the column means (false: from 0 -- no intercept, no standardisation)
  const double* scale = nullptr;       // p: the sd the driver standardises feature j with (1 where it does not)
  bool fit_intercept = true;           // false: the last coordinate stays at b0
  double b0 = 0.0;                     // the null model's intercept: where the path starts
  int device = 0;
  // the path, in the driver's units (regularization_path): l2 strength alpha[l], l1 strength beta[l]
  int n_lambda = 0;
  const double* alpha = nullptr;
  const double* beta = nullptr;
  bool ridge = false;                  // the ridge functor: no threshold
  unsigned max_iter = 0;               // outer steps per lambda
  double tol = 0.0;
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
};

// The Newton loop (newton.hip).  p <= kNewtonMaxFeatures is the caller's business (plan_fit).  timed: fill the *_ms fields.
int newton_run(const NewtonProblem& pb, bool timed, NewtonResult* out);

// Diagnostics (include/sgdnet_hip.h: sgdnet_newton_probe_*): one outer step through the host steps newton_run takes, every
// output copied back.  pb: x, y, centre, scale, device and n_lambda = 1; the rest comes from io.  The caller has checked both.
int newton_probe(const NewtonProblem& pb, sgdnet_newton_probe* io);

}  // namespace sgdnet
