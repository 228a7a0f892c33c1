// The matrix-core moments pass of wide Newton mode (newton_mfma.hip), as newton.hip launches it.  The geometry and the row
// split are wide_layout.hpp's (wide_mfma_*); the buffer bound is newton.hpp's.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sgdnet {

// M (ncols x ncols, ncols = p + 2) from the column-major n x p matrix x, the state pass's v and r and the centres mu: what
// newton_dense_tile_kernel and cov_reduce_kernel leave there, entry by entry, with the rows summed in another order.
// part: wide_mfma_partial_bytes(n, p + 2) bytes.  Two launches on st; the caller checks hipGetLastError.
void wnewton_mfma_moments(const double* x, const double* v, const double* r, const double* mu, int64_t n, int p, double* part, double* M,
                          hipStream_t st);

}  // namespace sgdnet
