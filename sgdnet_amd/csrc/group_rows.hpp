// The row chunks of the dense moments passes and the group-row layout of the cross-validated covariance modes: what
// driver_direct.cpp predicts a grid from and what covariance.hip launches it from.  No HIP type in here.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "wide_layout.hpp"

namespace sgdnet {

constexpr int64_t kMomentTileRows = 64;     // rows staged per step (moments_device.hpp: kTileRows)

// The narrow modes' rows of a chunk: moments_device.hpp's dense_rows_per_chunk in plain constexpr (that header is device
// code; tests/test_group_rows_host.py holds this one to the numpy restatement the pass tests cut their chunks by).  A
// function of n and the number of tile pairs alone: at most max(16, min(256, 1024 / pairs)) chunks, none shorter than 256
// rows, whole steps of tile_rows staged rows
constexpr int64_t narrow_rows_per_chunk(int64_t n, int64_t pairs, int64_t tile_rows) {
  const int64_t by_grid = 1024 / pairs < 256 ? 1024 / pairs : 256, cap = by_grid > 16 ? by_grid : 16;
  const int64_t by_rows = (n + 255) / 256, chunks = by_rows < cap ? by_rows : cap;
  return ((n + chunks - 1) / chunks + tile_rows - 1) / tile_rows * tile_rows;
}

// The rows of a chunk of a covariance-family moments pass over ncols columns of n rows (a fit: p + K; CV: p + K + 1)
constexpr int64_t cov_rows_per_chunk(int64_t n, int64_t ncols, bool wide) {
  return wide ? wide_rows_per_chunk(n, ncols, kMomentTileRows) : narrow_rows_per_chunk(n, wide_tile_pairs(ncols), kMomentTileRows);
}

// The row chunks of a dense group moments pass (gridDim.y): count[g] rows in group g, none across a group's end
inline int64_t group_row_chunks(const int64_t* count, int n_groups, int64_t rows_per_chunk) {
  int64_t chunks = 0;
  for (int g = 0; g < n_groups; ++g) chunks += (count[g] + rows_per_chunk - 1) / rows_per_chunk;
  return chunks;
}

// The rows sorted by group (stable: a group's rows stay in row order) and cut into chunks of rows_per_chunk rows, none
// across a group's end: chunk c is perm[chunk_begin[c] .. chunk_begin[c + 1]) and group g has the chunks
// [group_chunk[g], group_chunk[g + 1]).  chunk_begin ends with n.
struct GroupRows {
  std::vector<int64_t> perm, chunk_begin;
  std::vector<int32_t> group_chunk;
  size_t chunks() const { return chunk_begin.empty() ? 0 : chunk_begin.size() - 1; }
};

// fold[i] in [0, n_groups).  False, with nothing built, when there would be more than max_chunks chunks.
inline bool group_rows(const int32_t* fold, int64_t n, int n_groups, int64_t rows_per_chunk, int64_t max_chunks, GroupRows* out) {
  std::vector<int64_t> count((size_t)n_groups, 0);
  for (int64_t i = 0; i < n; ++i) ++count[(size_t)fold[i]];
  if (group_row_chunks(count.data(), n_groups, rows_per_chunk) > max_chunks) return false;
  std::vector<int64_t> fill((size_t)n_groups, 0);
  out->group_chunk.assign((size_t)n_groups + 1, 0);
  out->chunk_begin.clear();
  int64_t at = 0;
  for (int g = 0; g < n_groups; ++g) {
    fill[(size_t)g] = at;
    for (int64_t r = at; r < at + count[(size_t)g]; r += rows_per_chunk) out->chunk_begin.push_back(r);
    out->group_chunk[(size_t)g + 1] = (int32_t)out->chunk_begin.size();
    at += count[(size_t)g];
  }
  out->chunk_begin.push_back(n);
  out->perm.resize((size_t)n);
  for (int64_t i = 0; i < n; ++i) out->perm[(size_t)fill[(size_t)fold[i]]++] = i;
  return true;
}

}  // namespace sgdnet
