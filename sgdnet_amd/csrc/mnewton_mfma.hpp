// The matrix-core class-pair moments pass of wide multinomial Newton mode (mnewton_mfma.hip), as mnewton.hip launches it.
// The geometry, the class-pair groups and the buffer bound are mnewton.hpp's (wmnewton_mfma_*) over wide_layout.hpp's tiles.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sgdnet {

// M (K (K + 1) / 2 matrices of ncols x ncols, ncols = p + 2) from the column-major n x p matrix x, the class codes y, the
// state pass's mu (n x K, a column per class) and the centres m: what mnewton_pair_tile_kernel and
// mnewton_pair_reduce_kernel leave there, entry by entry, with the rows summed in another order.
// part: wmnewton_mfma_partial_bytes(n, p + 2, K) bytes.  Two launches on st; the caller checks hipGetLastError.
void wmnewton_mfma_moments(const double* x, const double* y, const double* mu, const double* m, int64_t n, int p, int K, double* part,
                           double* M, hipStream_t st);

}  // namespace sgdnet
