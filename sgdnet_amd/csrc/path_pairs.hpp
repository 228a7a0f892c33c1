// What the kernels that walk a whole lambda path share (score.hip, gradient.hip): a lane owns one
// (lambda, class) pair, a path is cut into chunks of lambdas whose pairs fit one kernel call, and the
// coefficients of a chunk are re-laid (p, lambda, class) so that one non-zero of a sample meets
// contiguous coefficients.
#pragma once

#include "common.hpp"

namespace sgdnet {
namespace {

constexpr int kMaxPairs = 1024;            // (lambda, class) pairs per call (LDS: 4 x 8 KB)
constexpr int kMaxLambda = 256;            // lambdas per call (4 running sums per lane)

// beta[k + K * (j + p * l)]  ->  B[(j * L + l) * K + k]
__global__ __launch_bounds__(256) void relayout_beta_kernel(const double* beta, int64_t p, int K, int L, double* B) {
  const int64_t total = p * (int64_t)L * K;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int k = (int)(t % K);
    const int64_t jl = t / K;
    const int l = (int)(jl % L);
    const int64_t j = jl / L;
    B[t] = beta[k + (int64_t)K * (j + p * l)];
  }
}

}  // namespace
}  // namespace sgdnet
