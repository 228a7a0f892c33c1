// The descent core the wide kernels share (covariance.hip: cov_wide_path_kernel, newton.hip: newton_wide_cd_kernel,
// mnewton.hip: mnewton_wide_cd_kernel): the scale kernel that writes their matrix to global memory (mnewton.hip has its
// own, over the class pairs), the ascending list compaction and the column move.  The geometry is wide_layout.hpp's.
// Included by those three units only, after moments_device.hpp; everything has internal linkage (each unit gets its own
// copy, as if it were written in it).
#pragma once

#include "moments_device.hpp"
#include "wide_layout.hpp"

namespace sgdnet {
namespace {

static_assert(kTileCols == 16 && kBlock == 256, "wide_tile_pairs and the partial-tile bounds count 16-column tiles of 256 partial sums");

// blockIdx.x = column j of the matrix A over the P = ncols - 1 coordinates: A[k + ld j] = M_jk / n / (s_j s_k), the
// arithmetic of the narrow kernels' prologues, from the upper triangle of the ncols x ncols moment matrix M; s = scale for
// the p features and 1 beyond them (newton's ones); rows P .. ld - 1 are the zero pad.  Also diag A, and the right-hand
// side from M's last column: rhs_j = M[j, ncols - 1] / n / s_j.
__global__ __launch_bounds__(kBlock) void wide_scale_kernel(const double* __restrict__ M, const double* __restrict__ scale, int p, int ncols,
                                                             int ld, double dn, double* __restrict__ A, double* __restrict__ Ad,
                                                             double* __restrict__ rhs) {
  const int j = blockIdx.x, P = ncols - 1;
  const double sj = j < p ? scale[j] : 1.0;
  for (int k = threadIdx.x; k < ld; k += kBlock) {
    double v = 0.0;
    if (k < P) {
      const double sk = k < p ? scale[k] : 1.0;
      v = k >= j ? M[(size_t)j * ncols + k] / dn / (sj * sk) : M[(size_t)k * ncols + j] / dn / (sk * sj);
    }
    A[(size_t)j * ld + k] = v;
    if (k == j) Ad[j] = v;
  }
  if (threadIdx.x == 0) rhs[j] = M[(size_t)j * ncols + P] / dn / sj;
}

// The list from one flag per coordinate, in ascending order; returns its length.  flag(j) is called by the lane that owns
// coordinate j, in every step for all kWidth lanes: it answers false for j >= count (the caller's own bound, so that the
// kernels compile to what they were with their own copies of this text: profiles/wide_core_resources.txt).  kWidth
// coordinates a step: a ballot per wavefront, the wavefronts' counts through LDS -- ascending whatever kWidth is, no atomic.
// A wavefront rewrites the bits of its own 64 coordinates (and flag may read them: they are read before the ballot).
template <int kWidth, class Flag>
__device__ __forceinline__ int wide_compact(int count, int32_t* list, uint32_t* bits, int32_t* counts, Flag flag) {
  constexpr int kWaves = kWidth / 64;
  static_assert(kWaves * 2 <= kWideScanWords, "the compaction's counts (wide_layout.hpp)");
  const int lane = threadIdx.x, wave = lane >> 6, wl = lane & 63;
  int length = 0, buf = 0;
  for (int base = 0; base < count; base += kWidth) {
    const int j = base + lane, first = base + wave * 64;
    const bool in = flag(j);
    const unsigned long long b = __ballot(in);
    if (wl == 0) counts[buf * kWaves + wave] = __popcll(b);
    __syncthreads();
    int before = 0, total = 0;
    for (int v = 0; v < kWaves; ++v) {
      const int n_v = counts[buf * kWaves + v];
      before += v < wave ? n_v : 0;
      total += n_v;
    }
    if (in) list[length + before + __popcll(b & ((1ull << wl) - 1ull))] = j;
    if (wl == 0 && first < count) {
      bits[first >> 5] = (uint32_t)b;
      if (first + 32 < count) bits[(first >> 5) + 1] = (uint32_t)(b >> 32);
    }
    length += total;
    buf ^= 1;        // (the counts of step i are read before the barrier of step i + 1 and rewritten behind it)
  }
  __syncthreads();
  return length;
}

// g[k] += A[k, j] d for all k < count, col = column j of A: a lane owns the slots s = lane, lane + kWidth, ...; a slot is
// k = 2 s and 2 s + 1, 16 bytes (count odd: the last one's second entry is A's zero pad, and g's is not touched).
template <int kWidth>
__device__ __forceinline__ void wide_column_move(double* g, const double* col, int count, double d) {
  const int slots = (count + 1) / 2;
#pragma unroll 4
  for (int s = threadIdx.x; s < slots; s += kWidth) {
    const int k = 2 * s;
    const double2 v = *reinterpret_cast<const double2*>(col + k);
    if (k + 1 < count) {
      double2 gk = *reinterpret_cast<double2*>(g + k);
      gk.x = fma(v.x, d, gk.x);
      gk.y = fma(v.y, d, gk.y);
      *reinterpret_cast<double2*>(g + k) = gk;
    } else {
      g[k] = fma(v.x, d, g[k]);
    }
  }
}

}  // namespace
}  // namespace sgdnet
