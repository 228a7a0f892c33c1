// The wide modes (SGDNET_MODE_WCOVARIANCE, SGDNET_MODE_WNEWTON): the geometry covariance.hpp and newton.hpp share.
// No HIP type in here: both are included by fit_plan.hpp.
//
// A wide kernel (covariance.hip: cov_wide_path_kernel, newton.hip: newton_wide_cd_kernel) is ONE workgroup that keeps a few
// f64 vectors over its `count` coordinates in LDS (the mode's own: covariance.hpp has four over p, newton.hpp three over
// P = p + 1) and, for the descent core of wide_cd_device.hpp,
//   the ascending list of the coordinates that may move, int32        count words
//   one bit per coordinate: "is in the list" (a coordinate of the
//   list may come to rest at 0, so a value != 0 does not say it)      ceil(count / 32) words
//   the wavefronts' counts of a list compaction step, twice           2 x 16 words
// and nothing of size count^2: the matrix is a full symmetric one in global memory whose leading dimension is count rounded
// up to 16 doubles (every column starts on a 128-byte line; the pad is zero), written by wide_scale_kernel.
#pragma once

#include <stdint.h>

namespace sgdnet {
#pragma GCC visibility push(hidden)     // (the library exports none of these)

constexpr int kWideLdsBytes = 160 * 1024;     // a workgroup of gfx950 may declare the CU's whole LDS
constexpr int kWideScanWords = 2 * 16;
constexpr int wide_list_bytes(int count) { return 4 * count + 4 * ((count + 31) / 32) + 4 * kWideScanWords; }
constexpr int64_t wide_leading_dim(int64_t count) { return (count + 15) / 16 * 16; }

// The kernels' workgroup: a column of 198 doubles is less than one stride of 256 lanes, and twelve more wavefronts only
// wait at the barriers; from 1000 features on sixteen wavefronts win (the tables of covariance.hip and newton.hip).
constexpr int kWideNarrow = 256, kWideFull = 1024;
constexpr int wide_cd_width(int p) { return p <= 512 ? kWideNarrow : kWideFull; }

// The dense moments pass over ncols columns (x, the response or the ones, ...): its partial-tile buffer holds chunks x tile
// pairs x 256 doubles.  The row chunks are a function of n and ncols alone: as many as it takes to put 1024 workgroups on
// the GPU (256 CUs x 4), none shorter than 256 rows, and ONE once the tile pairs alone are that many -- so the buffer is
// 2 MiB while there are chunks and pairs x 2 KiB beyond.
constexpr int64_t wide_tile_pairs(int64_t ncols) { return ((ncols + 15) / 16) * ((ncols + 15) / 16 + 1) / 2; }
constexpr int64_t wide_row_chunks(int64_t n, int64_t ncols) {
  const int64_t pairs = wide_tile_pairs(ncols), cap = pairs >= 1024 ? 1 : 1024 / pairs, by_rows = (n + 255) / 256;
  return by_rows < 1 ? 1 : (by_rows < cap ? by_rows : cap);
}
// the rows of a chunk: n over the chunks, rounded up to whole steps of tile_rows staged rows
constexpr int64_t wide_rows_per_chunk(int64_t n, int64_t ncols, int64_t tile_rows) {
  return ((n + wide_row_chunks(n, ncols) - 1) / wide_row_chunks(n, ncols) + tile_rows - 1) / tile_rows * tile_rows;
}

#pragma GCC visibility pop
}  // namespace sgdnet
