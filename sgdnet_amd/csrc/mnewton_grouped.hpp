// The inner solves and the publish of the multinomial Newton modes under the grouped penalty (mnewton_grouped.hip), as
// mnewton.hip's MNewtonDevice launches them where MNewtonProblem::grouped is set.  The LDS accounting is mnewton.hpp's
// (mnewton_grouped_state_doubles, wmnewton_grouped_state_bytes).  One launch each on st; the caller checks hipGetLastError.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sgdnet {

// mnewton_cd_kernel's arguments without `ridge` (alpha = 0 runs the ungrouped kernels); width: 64 or 256 lanes
void mnewton_grouped_cd(int width, const double* M, const double* scale, int p, int K, double dn, const double* u_cur, double al, double be,
                        int fit_intercept, unsigned max_sweeps, double tol, double* u_cand, double* a_cand, double* rec, hipStream_t st);

// mnewton_wide_cd_kernel's arguments without `ridge`, on what mnewton_wide_scale_kernel wrote; width: 256 or 1024 lanes
void mnewton_wide_grouped_cd(int width, const double* H, const double* Hd, const double* q, const double* scale, int p, int K, int ld,
                             const double* u_cur, double al, double be, int fit_intercept, unsigned max_sweeps, double tol, double* u_cand,
                             double* a_cand, double* rec, hipStream_t st);

// mnewton_blend_kernel / mnewton_wide_blend_kernel with sum_j |w_.j|_2 in the record's kRecAbs
void mnewton_grouped_blend(bool wide, const double* u_cur, const double* scale, int p, int Q, double t, double* u_cand, double* a_cand,
                           double* rec, hipStream_t st);

}  // namespace sgdnet
