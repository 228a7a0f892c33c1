// The fit driver behind sgdnet_fit_* / sgdnet_cv_* (include/sgdnet_hip.h) as its own translation units see it:
//   driver.cpp          validation, preprocessing, the lambda path, the plan's SAGA stages, the setup probes
//   driver_direct.cpp   the direct modes (fit_plan.hpp: is_direct_mode): their stages behind the plan, both
//                       cross-validation drivers and the Newton probes -- nothing in it touches a SAGA solver
// Private to those two files; none of it is a symbol of the library.
#pragma once

#include <stdio.h>
#include <stdlib.h>

#include <chrono>
#include <thread>
#include <vector>

#include "common.hpp"
#include "fit_plan.hpp"
#include "setup_device.hpp"

namespace sgdnet {
#pragma GCC visibility push(hidden)

// SGDNET_TRACE=1: wall-clock of the driver's phases on stderr
struct PhaseTimer {
  bool on;
  std::chrono::steady_clock::time_point t0;
  PhaseTimer() : on(getenv("SGDNET_TRACE") != nullptr), t0(std::chrono::steady_clock::now()) {}
  void mark(const char* what) {
    if (!on) return;
    const auto t1 = std::chrono::steady_clock::now();
    fprintf(stderr, "[sgdnet] %-28s %8.3f s\n", what, std::chrono::duration<double>(t1 - t0).count());
    t0 = t1;
  }
};

struct Features {
  bool sparse = false;
  int64_t n = 0, p = 0;
  // feature-major (as passed by R), preprocessed values
  const int32_t* colptr = nullptr;
  const int32_t* rowidx = nullptr;
  std::vector<double> val;      // sparse values (scaled if standardize)
  std::vector<double> xd;       // dense n x p column-major (standardised if requested)
  // sample-major
  std::vector<int64_t> sptr;
  std::vector<int32_t> sidx;
  std::vector<double> sval;
  std::vector<double> xt;       // dense p x n
  std::vector<double> x_center, x_scale, x_center_scaled;
  // device-side setup (sparse): the O(nnz) passes run in setup_device.hip and the vectors
  // above other than x_center / x_scale stay empty
  DeviceSetup* dev = nullptr;
  hipStream_t st = nullptr;
  double dev_max_mean_sq = 0.0;
  bool dense_dev = false;       // dense x prepared by dense_setup_* (large matrices)
  // x as it came (the direct modes take their moments from it): the column-major matrix, or the dgCMatrix values
  const double* raw_dense = nullptr;
  const double* raw_values = nullptr;
};

struct Response {
  std::vector<double> y;                   // n x Ky, preprocessed
  std::vector<double> yt;                  // Ky x n, preprocessed: what the solvers read
  std::vector<double> y_center, y_scale;
  std::vector<double> b0;                  // the null model's intercept
  double null_dev_scaled = 0.0;            // null deviance of the preprocessed response
};

struct Path {
  std::vector<double> lambda, alpha, beta;
};

// Host-side passes over dense x (R hands over a column-major matrix): per-column work is split
// over a few threads.  Every column is still reduced by one thread in the reference's order, so
// the results are bitwise those of the serial loops.
template <class F>
void parallel_for(int64_t count, double work, F f) {
  unsigned T = std::thread::hardware_concurrency();
  if (T > 16) T = 16;
  if (work < 4e6 || T < 2 || count < 2) {
    f((int64_t)0, count);
    return;
  }
  if ((int64_t)T > count) T = (unsigned)count;
  std::vector<std::thread> th;
  for (unsigned t = 0; t < T; ++t) {
    const int64_t lo = count * t / T, hi = count * (t + 1) / T;
    th.emplace_back([=, &f] { f(lo, hi); });
  }
  for (auto& x : th) x.join();
}

// ---- driver.cpp ----
double binomial_link(double ybar);
int validate_response(const sgdnet_control* c, const double* y, int64_t n);
int validate_colptr(const sgdnet_csc* x);
int validate_rowidx(const sgdnet_csc* x);
// a HIP device is there and `device` is one of them
int check_device(int device);
// Rescale (utils.h:352-378): the coefficients of lambda li on the scale of the data as it came
// w (K x p) and b (K): the coefficients and intercepts of the preprocessed problem
void rescale_values(const Features& X, const Response& R, const sgdnet_control* ctl, int li, const double* w, const double* b,
                    sgdnet_result* out);

// ---- driver_direct.cpp ----
// the stage behind a direct mode's plan: the whole path, from x as it came
int fit_direct(const Features& X, const Response& R, const Path& path, const FitPlan& plan, const sgdnet_control* ctl, sgdnet_result* out,
               PhaseTimer& pt);

#pragma GCC visibility pop
}  // namespace sgdnet
