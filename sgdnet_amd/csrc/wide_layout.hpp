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

// The matrix-core moments pass of wide Newton mode (newton_mfma.hip; the option "wnewton_moments" = 1) over ncols = p + 2
// columns.  A workgroup owns a pair of macro tiles of kMfmaTileCols columns and steps through its rows in slabs of
// kMfmaSlabRows; its partial tile is kMfmaTileCols^2 doubles (32 KiB).  The row chunks are a function of n and ncols alone:
// as many as it takes to put 2048 workgroups on the GPU (256 CUs x 8 short ones balance better than x 4 long ones, and a
// chunk's partial tile costs 32 KiB of traffic against the 128 columns x rows it read), none shorter than
// kMfmaMinChunkRows, and ONE once two chunks of every macro-tile pair would be more than that (p + 2 > 2816).  Examples:
//   p + 2 <= 64 (one pair): a chunk per 256 rows up to 2048 chunks -- 256 rows 1, 257 rows 2 (the second holds one row),
//                           513 rows 3; beyond 524 288 rows the chunks grow instead
//   20000 x 1000 (136 pairs): 15 chunks of 1344 rows (the last holds 1184), 2040 workgroups
//   500 x 2000 (528 pairs):   3 chunks would be allowed, but 500 rows are 2 chunks of 256
//   the limit p = 5819 (4186 pairs): one chunk whatever n is
constexpr int kMfmaTileCols = 64, kMfmaSlabRows = 32, kMfmaMinChunkRows = 256, kMfmaWorkgroups = 2048;
constexpr int64_t wide_mfma_tiles(int64_t ncols) { return (ncols + kMfmaTileCols - 1) / kMfmaTileCols; }
constexpr int64_t wide_mfma_pairs(int64_t ncols) { return wide_mfma_tiles(ncols) * (wide_mfma_tiles(ncols) + 1) / 2; }
// macro-tile pair 0 .. wide_mfma_pairs - 1 -> (tI, tJ), tI <= tJ, row by row of the upper triangle (the kernels call it too)
constexpr void macro_pair(int pair, int tiles, int& tI, int& tJ) {
  tI = 0;
  while (pair >= tiles - tI) {
    pair -= tiles - tI;
    ++tI;
  }
  tJ = tI + pair;
}
// the rows of a chunk: n over the chunks the workgroup target allows, in whole slabs, at least kMfmaMinChunkRows.
// workgroups: those of ONE chunk (the macro-tile pairs; mnewton.hpp: times the class-pair groups)
constexpr int64_t wide_mfma_chunk_rows(int64_t n, int64_t workgroups) {
  const int64_t cap = workgroups >= kMfmaWorkgroups ? 1 : kMfmaWorkgroups / workgroups;
  const int64_t rows = ((n + cap - 1) / cap + kMfmaSlabRows - 1) / kMfmaSlabRows * kMfmaSlabRows;
  return rows < kMfmaMinChunkRows ? kMfmaMinChunkRows : rows;
}
constexpr int64_t wide_mfma_rows_per_chunk(int64_t n, int64_t ncols) { return wide_mfma_chunk_rows(n, wide_mfma_pairs(ncols)); }
constexpr int64_t wide_mfma_row_chunks(int64_t n, int64_t ncols) {
  return n < 1 ? 1 : (n + wide_mfma_rows_per_chunk(n, ncols) - 1) / wide_mfma_rows_per_chunk(n, ncols);
}
constexpr int64_t wide_mfma_partial_bytes(int64_t n, int64_t ncols) {
  return wide_mfma_row_chunks(n, ncols) * wide_mfma_pairs(ncols) * kMfmaTileCols * kMfmaTileCols * 8;
}
static_assert(wide_mfma_row_chunks(1, 3) == 1 && wide_mfma_row_chunks(256, 9) == 1 && wide_mfma_row_chunks(257, 9) == 2 &&
              wide_mfma_row_chunks(512, 9) == 2 && wide_mfma_row_chunks(513, 9) == 3, "a chunk per 256 rows at one pair");
static_assert(wide_mfma_row_chunks(524288, 64) == 2048 && wide_mfma_rows_per_chunk(524289, 64) == 288 &&
              wide_mfma_row_chunks(524289, 64) == 1821, "beyond 2048 chunks the chunks grow");
static_assert(wide_mfma_pairs(1002) == 136 && wide_mfma_rows_per_chunk(20000, 1002) == 1344 && wide_mfma_row_chunks(20000, 1002) == 15,
              "20000 x 1000");
static_assert(wide_mfma_pairs(2002) == 528 && wide_mfma_row_chunks(500, 2002) == 2, "500 x 2000");
static_assert(wide_mfma_pairs(2816) == 990 && wide_mfma_row_chunks(1 << 30, 2816) == 2 && wide_mfma_pairs(2817) == 1035 &&
              wide_mfma_row_chunks(1 << 30, 2817) == 1, "one chunk from 1025 pairs on");

#pragma GCC visibility pop
}  // namespace sgdnet
