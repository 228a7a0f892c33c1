// What every direct mode's problem holds (covariance.hpp, newton.hpp and mnewton.hpp derive theirs from it): x as it came,
// the preprocessing the driver applied, the device and the path.  No HIP type in here.
#pragma once

#include <stdint.h>

namespace sgdnet {

struct DirectProblem {
  int64_t n = 0, p = 0;
  // x as the fit entry points receive it: one of the two, in host memory
  const double* x_dense = nullptr;     // column-major n x p
  const int32_t* colptr = nullptr;     // dgCMatrix slots; row indices ascending within a column
  const int32_t* rowidx = nullptr;
  const double* values = nullptr;
  bool centre = true;                  // deviations from the column means (false: from 0 -- no intercept, no standardisation)
  const double* scale = nullptr;       // p: the sd the driver standardises feature j with (1 where it does not)
  int device = 0;
  // the path, in the driver's units (regularization_path): l2 strength alpha[l], l1 (or group) threshold beta[l]
  int n_lambda = 0;
  const double* alpha = nullptr;
  const double* beta = nullptr;
  bool ridge = false;                  // the ridge functor: no threshold
  unsigned max_iter = 0;               // per lambda: coordinate (block) sweeps, or outer steps of the Newton modes
  double tol = 0.0;
};

}  // namespace sgdnet
