// The moments pass of wide Newton mode on the f64 matrix cores (the option "wnewton_moments" = 1; newton.hip has the pass
// it replaces, newton_dense_tile_kernel + cov_reduce_kernel, and says what the moments are).  wide_mfma_device.hpp has the
// macro tile, the slab, the operand layout and the pipeline.  This unit's own: one weight per row, v and r of the state pass,
// so the B side is weighted once, as it is stored -- Bs[c][i] = v d, v in the ones column, r in column p + 1 -- and there is
// no weight table and one set of accumulators (2 wavefronts a SIMD).  The rows of a chunk are a plain range of [0, n):
// wide_layout.hpp: wide_mfma_rows_per_chunk.  The reduce kernel writes entry for entry what cov_reduce_kernel writes.
#include "newton_mfma.hpp"

#include "wide_mfma_device.hpp"

namespace sgdnet {
namespace {

__global__ __launch_bounds__(kLanes) void newton_mfma_tile_kernel(const double* __restrict__ x, const double* __restrict__ v,
                                                                   const double* __restrict__ r, const double* __restrict__ mu,
                                                                   int64_t n, int p, int64_t rows_per_chunk, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) slab_t As;
  __shared__ __attribute__((aligned(16))) slab_t Bs;
  const MfmaTile L(p + 2, rows_per_chunk, n);
  MfmaColumns X(L, mu, p);
  double vi = 0.0, ri = 0.0;
  auto load = [&](int64_t base) {
    const int64_t i = base + L.srow;
    const bool live = i < L.r1;
    vi = live ? v[i] : 0.0;
    ri = live ? r[i] : 0.0;
    X.load(L, x, n, p, i, live);
  };
  auto store = [&]() {                     // centred, then weighted, as newton_dense_tile_kernel stages them
    X.store(L, As, Bs, p, [&](int b, double d) { return b == p + 1 ? ri : vi * d; });
  };
  acc_t acc[2][2];
  for (int ta = 0; ta < 2; ++ta)
    for (int tb = 0; tb < 2; ++tb) acc[ta][tb] = acc_t{0.0, 0.0, 0.0, 0.0};
  mfma_slabs(L, load, store, [&]() {
    double fa[2][8], fb[2][8];
    mfma_fragments(L, As, Bs, fa, fb);
    mfma_block(fa, fb, acc);
  });
  if (!L.idle) mfma_store_tile(L, part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (size_t)(kT * kT), acc);
}

// blockIdx.x = macro-tile pair; part[chunk][macro pair][64 x 64]
__global__ __launch_bounds__(kLanes) void newton_mfma_reduce_kernel(const double* __restrict__ part, int chunks, int ncols,
                                                                     double* __restrict__ M) {
  mfma_reduce(part + (size_t)blockIdx.x * (size_t)(kT * kT), (size_t)gridDim.x * (size_t)(kT * kT), chunks, ncols, M);
}

}  // namespace

void wnewton_mfma_moments(const double* x, const double* v, const double* r, const double* mu, int64_t n, int p, double* part, double* M,
                          hipStream_t st) {
  const int ncols = p + 2;
  const int64_t pairs = wide_mfma_pairs(ncols), rows = wide_mfma_rows_per_chunk(n, ncols), chunks = wide_mfma_row_chunks(n, ncols);
  hipLaunchKernelGGL(newton_mfma_tile_kernel, dim3((unsigned)pairs, (unsigned)chunks), dim3(kLanes), 0, st, x, v, r, mu, n, p, rows, part);
  hipLaunchKernelGGL(newton_mfma_reduce_kernel, dim3((unsigned)pairs), dim3(kLanes), 0, st, part, (int)chunks, ncols, M);
}

}  // namespace sgdnet
