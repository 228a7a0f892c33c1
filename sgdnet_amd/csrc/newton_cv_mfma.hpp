// The moments pass of the wide Newton cross-validation on the f64 matrix cores (newton_cv_mfma.hip; the option
// "cv_wnewton_moments" = 1): what newton.hip's lock-step loop launches in place of newton_cv_dense_tile_kernel +
// newton_cv_reduce_kernel.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

#include "newton_cv_device.hpp"

namespace sgdnet {

// cmd, jobs: the round's commands and the jobs' geometry, job (mix a, set t) = a * n_sets + t, whose rows_per_chunk and
// chunks are the matrix-core ones (newton.hpp: wnewton_cv_mfma_*); x: column-major n x p with the rows sorted by group;
// v_all, r_all: jobs x n; mu_all: n_sets x p; part: jobs x max_chunks x wide_mfma_pairs(p + 2) x 64 x 64; M_all: jobs x
// (p + 2)^2.  Only the M of a job whose command is kCvStep is written.  Device pointers.
void wnewton_cv_mfma_moments(const CvCmd* cmd, const CvJob* jobs, const double* x, const double* v_all, const double* r_all,
                             const double* mu_all, int64_t n, int p, int n_sets, int n_mix, int max_chunks, double* part, double* M_all,
                             hipStream_t st);

}  // namespace sgdnet
