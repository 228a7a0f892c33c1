// The class-pair moments pass of the wide multinomial Newton cross-validation on the f64 matrix cores (mnewton_cv_mfma.hip;
// the option "cv_wmnewton_moments" = 1): what mnewton.hip's lock-step loop launches in place of mnewton_cv_pair_tile_kernel +
// mnewton_cv_pair_reduce_kernel.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

#include "newton_cv_device.hpp"

namespace sgdnet {

// cmd, jobs: the round's commands and the jobs' geometry, job (mix a, set t) = a * n_sets + t, whose rows_per_chunk and
// chunks are the matrix-core ones (mnewton.hpp: wmnewton_mfma_rows_per_chunk of n_t rows); mu_at: where a job's mu starts in
// mu_all (by the job's local row, a column per class); x: column-major n x p with the rows sorted by group; y: n class
// codes; m_all: n_sets x p; part: jobs x class pairs x max_chunks x wide_mfma_pairs(p + 2) x 64 x 64; M_all: jobs x class
// pairs x (p + 2)^2.  Only the matrices of a job whose command is kCvStep are written.  Device pointers.  Two launches on
// st; the caller checks hipGetLastError.
void wmnewton_cv_mfma_moments(const CvCmd* cmd, const CvJob* jobs, const int64_t* mu_at, const double* x, const double* y,
                              const double* mu_all, const double* m_all, int64_t n, int p, int K, int n_sets, int n_mix, int max_chunks,
                              double* part, double* M_all, hipStream_t st);

}  // namespace sgdnet
