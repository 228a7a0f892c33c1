// The class-pair moments pass of wide multinomial Newton mode on the f64 matrix cores (the option "wmnewton_moments" = 1;
// mnewton.hip has the pass it replaces, mnewton_pair_tile_kernel + mnewton_pair_reduce_kernel, and says what the moments are).
//
// For every class pair c = (k <= l): M_c(a, b) = sum_i A(i, a) B_c(i, b) with A = [x - m | 1 | 0], B_c = [v_c (x - m) | v_c | r_c].
// All K (K + 1) / 2 matrices are Gram matrices of the SAME centred rows under another weight per row, so this is the grouped
// tile of wide_mfma_device.hpp, which has the geometry.  This unit's own:
//   rows         a plain range of [0, n); mnewton.hpp: wmnewton_mfma_rows_per_chunk, over macro pairs x groups workgroups a
//                chunk
//   weights      formed from mu and y (ClassPairWeights)
//   members      kG = kWmnewtonMfmaGroup consecutive class pairs (blockIdx.z); the last group of a K may be partial
//   tiles        part[chunk][class pair][macro pair]; the reduce kernel writes each pair's matrix entry for entry as
//                mnewton_pair_reduce_kernel does
#include "mnewton_mfma.hpp"

#include "mnewton.hpp"
#include "wide_mfma_device.hpp"

namespace sgdnet {
namespace {

constexpr int kG = kWmnewtonMfmaGroup;

struct FitClassPairs : ClassPairWeights {
  int c0, present, class_pairs;          // the group's first class pair, how many it has, and all of the fit
  double* part;
  __device__ bool member(int g) const { return g < present; }
  __device__ int64_t row(int64_t li, bool) const { return li; }
  __device__ double* tile(int g) const {
    return part + (((size_t)blockIdx.y * (size_t)class_pairs + (size_t)(c0 + g)) * gridDim.x + blockIdx.x) * (size_t)(kT * kT);
  }
};

__global__ __launch_bounds__(kLanes) void mnewton_mfma_tile_kernel(const double* __restrict__ x, const double* __restrict__ y,
                                                                    const double* __restrict__ mu, const double* __restrict__ m, int64_t n,
                                                                    int p, int K, int64_t rows_per_chunk, double* __restrict__ part) {
  const MfmaTile L(p + 2, rows_per_chunk, n);
  FitClassPairs G;
  G.class_pairs = K * (K + 1) / 2;
  G.c0 = (int)blockIdx.z * kG;
  G.present = G.class_pairs - G.c0 < kG ? G.class_pairs - G.c0 : kG;
  G.part = part;
  G.weigh = L.cg < G.present;
  G.ck = G.cl = 0;
  if (G.weigh) class_pair(G.c0 + L.cg, K, &G.ck, &G.cl);
  G.mu_k = mu + (int64_t)G.ck * n;
  G.mu_l = mu + (int64_t)G.cl * n;
  G.y = y;
  mfma_group_tile<kG>(L, G, x, m, n, p);
}

// blockIdx.x = macro-tile pair, blockIdx.y = class pair
__global__ __launch_bounds__(kLanes) void mnewton_mfma_reduce_kernel(const double* __restrict__ part, int chunks, int ncols,
                                                                      double* __restrict__ M_all) {
  const size_t tile = (size_t)(kT * kT);
  mfma_reduce(part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * tile, (size_t)gridDim.y * gridDim.x * tile, chunks, ncols,
              M_all + (size_t)blockIdx.y * (size_t)ncols * (size_t)ncols);
}

}  // namespace

void wmnewton_mfma_moments(const double* x, const double* y, const double* mu, const double* m, int64_t n, int p, int K, double* part,
                           double* M, hipStream_t st) {
  const int ncols = p + 2, class_pairs = K * (K + 1) / 2;
  const int64_t pairs = wide_mfma_pairs(ncols), groups = wmnewton_mfma_groups(K);
  const int64_t rows = wmnewton_mfma_rows_per_chunk(n, ncols, K), chunks = wmnewton_mfma_row_chunks(n, ncols, K);
  hipLaunchKernelGGL(mnewton_mfma_tile_kernel, dim3((unsigned)pairs, (unsigned)chunks, (unsigned)groups), dim3(kLanes), 0, st, x, y, mu, m, n,
                     p, K, rows, part);
  hipLaunchKernelGGL(mnewton_mfma_reduce_kernel, dim3((unsigned)pairs, (unsigned)class_pairs), dim3(kLanes), 0, st, part, (int)chunks, ncols, M);
}

}  // namespace sgdnet
