// What the moment passes of covariance.hip, newton.hip and mnewton.hip share: the tile geometry, the fixed-order workgroup sum, the
// column means, the chunk reduction, the row lookup of the sparse pair kernels, the packed triangle, and the host
// helpers around them.  Included by those three units only; everything has internal linkage (each unit gets its own
// copy of the kernels, as if they were written in it).
#pragma once

#include <algorithm>
#include <numeric>
#include <vector>

#include "common.hpp"

namespace sgdnet {
namespace {

constexpr int kBlock = 256;
constexpr int kTileCols = 16;     // columns per tile: 16 x 16 threads own a tile pair
constexpr int kTileRows = 64;     // rows staged per step

// the sum of v over the workgroup, in a fixed tree order; every thread gets it
__device__ double block_sum(double v, double* sh) {
  __syncthreads();
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  return sh[0];
}

// blockIdx.x = column j < p: mu[j] = mean of the column (sparse: over all n samples); column p + r, r < nresp: mu[p + r] =
// sum of response r (y is n x nresp, column-major).  One response: mu[p + 1] = mean of y as well (the centre of the
// response of the group moments)
template <bool kSparse>
__global__ __launch_bounds__(kBlock) void cov_sum_kernel(const double* __restrict__ x, const int32_t* __restrict__ colptr,
                                                          const double* __restrict__ y, int64_t n, int p, int nresp, int centre,
                                                          double* __restrict__ mu) {
  __shared__ double sh[kBlock];
  const int j = blockIdx.x;
  double s = 0.0;
  if (j >= p) {
    const double* col = y + (int64_t)(j - p) * n;
    for (int64_t i = threadIdx.x; i < n; i += kBlock) s += col[i];
  } else if (!centre) {
    // deviations from 0
  } else if (kSparse) {
    for (int64_t q = (int64_t)colptr[j] + threadIdx.x; q < colptr[j + 1]; q += kBlock) s += x[q];
  } else {
    const double* col = x + (int64_t)j * n;
    for (int64_t i = threadIdx.x; i < n; i += kBlock) s += col[i];
  }
  s = block_sum(s, sh);
  if (threadIdx.x == 0) {
    mu[j] = j >= p ? s : s / (double)n;
    if (j == p && nresp == 1) mu[p + 1] = s / (double)n;
  }
}

// the chunks' partial tiles added in chunk order; M is the symmetric ncols x ncols matrix of the augmented rows.
// blockIdx.y = group: its chunks are [group_chunk[g], group_chunk[g + 1]) and its matrix is M[g] (one fit: all chunks, M[0])
__global__ __launch_bounds__(kBlock) void cov_reduce_kernel(const double* __restrict__ part, int chunks,
                                                             const int32_t* __restrict__ group_chunk, int ncols, double* __restrict__ M) {
  const int tid = threadIdx.x;
  const int T = (ncols + kTileCols - 1) / kTileCols;
  int pair = blockIdx.x, tj = 0;
  while (pair >= T - tj) {
    pair -= T - tj;
    ++tj;
  }
  const int tk = tj + pair;
  const int a = tj * kTileCols + (tid & (kTileCols - 1)), b = tk * kTileCols + tid / kTileCols;
  if (a >= ncols || b >= ncols) return;
  const int c0 = group_chunk ? group_chunk[blockIdx.y] : 0, c1 = group_chunk ? group_chunk[blockIdx.y + 1] : chunks;
  M += (size_t)blockIdx.y * (size_t)ncols * (size_t)ncols;
  double s = 0.0;
  for (int c = c0; c < c1; ++c) s += part[((size_t)c * gridDim.x + blockIdx.x) * kBlock + tid];
  M[(size_t)a * ncols + b] = s;
  if (tj != tk) M[(size_t)b * ncols + a] = s;
}

// first position in rowidx[lo, hi) whose row is >= r
__device__ int lower_bound_row(const int32_t* __restrict__ rowidx, int lo, int hi, int32_t r) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (rowidx[mid] < r) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// S(j, k) of the packed triangle, j <= k
__device__ __forceinline__ int tri(int j, int k) { return k * (k + 1) / 2 + j; }

// one device allocation cut into aligned pieces
struct Arena {
  char* base = nullptr;
  size_t used = 0;
  ~Arena() {
    if (base) (void)hipFree(base);
  }
  size_t reserve(size_t bytes) {
    const size_t at = used;
    used += (bytes + 255) & ~(size_t)255;
    return at;
  }
  template <class T>
  T* at(size_t off) const { return reinterpret_cast<T*>(base + off); }
};

// the pair kernel looks rows up by binary search: columns whose row indices do not ascend are sorted in a copy
struct AscendingColumns {
  const int32_t* rowidx;
  const double* values;
  std::vector<int32_t> rows_sorted;
  std::vector<double> vals_sorted;
  AscendingColumns(const int32_t* colptr, const int32_t* rowidx_in, const double* values_in, int p) : rowidx(rowidx_in), values(values_in) {
    const int64_t nnz = p > 0 ? colptr[p] : 0;
    bool ascending = true;
    for (int j = 0; j < p && ascending; ++j)
      for (int64_t q = (int64_t)colptr[j] + 1; q < colptr[j + 1]; ++q)
        if (rowidx[q] <= rowidx[q - 1]) {
          ascending = false;
          break;
        }
    if (ascending) return;
    rows_sorted.assign(rowidx, rowidx + nnz);
    vals_sorted.assign(values, values + nnz);
    std::vector<int64_t> order;
    for (int j = 0; j < p; ++j) {
      const int64_t q0 = colptr[j], q1 = colptr[j + 1];
      order.resize((size_t)(q1 - q0));
      std::iota(order.begin(), order.end(), q0);
      std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return rowidx[a] < rowidx[b]; });
      for (int64_t q = q0; q < q1; ++q) {
        rows_sorted[(size_t)q] = rowidx[order[(size_t)(q - q0)]];
        vals_sorted[(size_t)q] = values[order[(size_t)(q - q0)]];
      }
    }
    rowidx = rows_sorted.data();
    values = vals_sorted.data();
  }
};

// dense x: the rows one chunk of the moments pass takes (a function of n and the number of tile pairs alone)
int64_t dense_rows_per_chunk(int64_t n, int pairs) {
  const int64_t chunk_cap = std::max<int64_t>(16, std::min<int64_t>(256, 1024 / pairs));
  const int64_t chunks = std::min<int64_t>(chunk_cap, (n + 255) / 256);
  return ((n + chunks - 1) / chunks + kTileRows - 1) / kTileRows * kTileRows;
}

}  // namespace
}  // namespace sgdnet
