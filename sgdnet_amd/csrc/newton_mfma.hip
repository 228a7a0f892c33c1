// The moments pass of wide Newton mode on the f64 matrix cores (the option "wnewton_moments" = 1; newton.hip has the pass
// it replaces, newton_dense_tile_kernel + cov_reduce_kernel, and says what the moments are).
//
// M(a, b) = sum_i A(i, a) B(i, b) over the ncols = p + 2 columns A = [x - mu | 1 | 0], B = [v (x - mu) | v | r].  Every
// term is formed as the old pass forms it -- d = x - mu rounded, then v d rounded -- and only then multiplied and
// accumulated by v_mfma_f64_16x16x4_f64 (a fused multiply-add per term); only the order of the sum over the rows differs.
//
//   macro tile   a workgroup of 256 lanes (4 wavefronts) owns the 64 x 64 entries (a, b) of one pair of 64-column macro
//                tiles (tI <= tJ; blockIdx.x) over one chunk of rows (blockIdx.y); wavefront w owns the 32 x 32 block
//                (w / 2, w % 2) of it as 2 x 2 accumulators of 16 x 16: 4 x 4 doubles a lane.  On a diagonal pair the
//                block (1, 0) lies below the diagonal 16-column tiles and is left out.
//   slab         32 rows of the 64 A columns and the 64 B columns, staged in LDS column by column with a stride of 34
//                doubles: As[c][i] = A(i, c), Bs[c][i] = B(i, c), centred and weighted once, as they are stored.  x is
//                column-major: lane t loads row t % 32 of the columns t / 32 + 8 j, 32 consecutive doubles a column.  A
//                diagonal pair loads its columns once and stores both forms.
//   operands     the instruction multiplies a 16 x 4 by a 4 x 16 block: lane l supplies A[l % 16][l / 16] and
//                B[l / 16][l % 16] and holds D[4 e + l / 16][l % 16] in element e of its accumulator.  The order of the
//                rows within a slab is free as long as A and B agree, so lane group g = l / 16 takes the rows 8 g .. 8 g + 7
//                in the slab's 8 steps: a lane reads its 8 rows of a column as four 16-byte LDS loads.  Stride 34: the 16
//                lanes of a group read 16 columns 272 bytes apart, 17 x 16 bytes: every 16-byte bank group once.
//   overlap      the global loads of slab s + 1 are issued into registers before the 32 matrix instructions of slab s and
//                are centred, weighted and stored to LDS after them (one LDS buffer, two barriers a slab).
//   row chunks   wide_layout.hpp: wide_mfma_rows_per_chunk; every workgroup stores its 64 x 64 partial tile, and
//                newton_mfma_reduce_kernel adds the chunks in chunk order into M: the 16-column tiles on or above the
//                diagonal, mirrored unless on it -- entry for entry what cov_reduce_kernel writes (a diagonal 16-column
//                tile holds both of its triangles as computed: M(p + 1, .) = 0 there, M(., p + 1) = q).
// No atomic, and the order of every sum is fixed by (n, p): the same input gives the same bits.
#include "newton_mfma.hpp"

#include "wide_layout.hpp"

namespace sgdnet {
namespace {

constexpr int kT = kMfmaTileCols, kS = kMfmaSlabRows, kLanes = 256;
constexpr int kStride = kS + 2;                      // doubles between two columns of a slab in LDS
constexpr int kColsPerLane = kT * kS / kLanes;       // 8: the columns of either side a lane stages
static_assert(kT == 64 && kS == 32 && kLanes == 256, "4 wavefronts x (2 x 2) tiles of 16 columns; 4 lane groups x 8 rows");
static_assert(kStride % 2 == 0 && (kStride / 2) % 16 == 1, "16-byte LDS loads: 16 columns fall into 16 different bank groups");

typedef double acc_t __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(kLanes) void newton_mfma_tile_kernel(const double* __restrict__ x, const double* __restrict__ v,
                                                                   const double* __restrict__ r, const double* __restrict__ mu,
                                                                   int64_t n, int p, int64_t rows_per_chunk, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) double As[kT][kStride], Bs[kT][kStride];
  const int tid = threadIdx.x, ncols = p + 2;
  int tI, tJ;
  macro_pair(blockIdx.x, (ncols + kT - 1) / kT, tI, tJ);
  const bool diag = tI == tJ;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_chunk;
  const int64_t r1 = r0 + rows_per_chunk < n ? r0 + rows_per_chunk : n;

  // staging: row `srow` of the slab, the columns cg + 8 j of either macro tile
  const int srow = tid & (kS - 1), cg = tid / kS;
  double muA[kColsPerLane], muB[kColsPerLane];
  for (int j = 0; j < kColsPerLane; ++j) {
    const int a = tI * kT + cg + 8 * j, b = tJ * kT + cg + 8 * j;
    muA[j] = a < p ? mu[a] : 0.0;
    muB[j] = b < p ? mu[b] : 0.0;
  }
  double xa[kColsPerLane], xb[kColsPerLane], vi = 0.0, ri = 0.0;
  bool live = false;
  auto load = [&](int64_t base) {          // the slab's values into registers; nothing outside the chunk or x is read
    const int64_t i = base + srow;
    live = i < r1;
    vi = live ? v[i] : 0.0;
    ri = live ? r[i] : 0.0;
#pragma unroll
    for (int j = 0; j < kColsPerLane; ++j) {
      const int a = tI * kT + cg + 8 * j, b = tJ * kT + cg + 8 * j;
      xa[j] = live && a < p ? x[i + (int64_t)a * n] : 0.0;
      xb[j] = !diag && live && b < p ? x[i + (int64_t)b * n] : 0.0;
    }
  };
  auto store = [&]() {                     // centred, then weighted, as newton_dense_tile_kernel stages them
#pragma unroll
    for (int j = 0; j < kColsPerLane; ++j) {
      const int c = cg + 8 * j, a = tI * kT + c, b = tJ * kT + c;
      const double da = a < p ? xa[j] - muA[j] : (a == p ? 1.0 : 0.0);
      const double db = b < p ? (diag ? xa[j] : xb[j]) - muB[j] : (b == p ? 1.0 : 0.0);
      As[c][srow] = live ? da : 0.0;
      Bs[c][srow] = live ? (b == p + 1 ? ri : vi * db) : 0.0;
    }
  };

  // the matrix instructions: lane group g takes the rows 8 g .. 8 g + 7 of the slab, column l % 16 of each 16-column tile
  const int wave = tid >> 6, lane = tid & 63, lc = lane & 15, lg = lane >> 4;
  const int wa = wave >> 1, wb = wave & 1;
  const bool idle = diag && wa > wb;       // below the diagonal 16-column tiles
  acc_t acc[2][2];
  for (int ta = 0; ta < 2; ++ta)
    for (int tb = 0; tb < 2; ++tb) acc[ta][tb] = acc_t{0.0, 0.0, 0.0, 0.0};

  load(r0);
  for (int64_t base = r0; base < r1; base += kS) {
    store();
    __syncthreads();
    if (base + kS < r1) load(base + kS);
    if (!idle) {
      double fa[2][8], fb[2][8];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const double2* pa = reinterpret_cast<const double2*>(&As[wa * 32 + t * 16 + lc][lg * 8]);
        const double2* pb = reinterpret_cast<const double2*>(&Bs[wb * 32 + t * 16 + lc][lg * 8]);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const double2 qa = pa[s], qb = pb[s];
          fa[t][2 * s] = qa.x;
          fa[t][2 * s + 1] = qa.y;
          fb[t][2 * s] = qb.x;
          fb[t][2 * s + 1] = qb.y;
        }
      }
#pragma unroll
      for (int s = 0; s < 8; ++s)
#pragma unroll
        for (int ta = 0; ta < 2; ++ta)
#pragma unroll
          for (int tb = 0; tb < 2; ++tb)
            acc[ta][tb] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[ta][s], fb[tb][s], acc[ta][tb], 0, 0, 0);
    }
    __syncthreads();
  }
  if (idle) return;
  double* out = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (size_t)(kT * kT);
#pragma unroll
  for (int ta = 0; ta < 2; ++ta)
#pragma unroll
    for (int tb = 0; tb < 2; ++tb)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        out[(wa * 32 + ta * 16 + 4 * e + lg) * kT + wb * 32 + tb * 16 + lc] = acc[ta][tb][e];
}

// blockIdx.x = macro-tile pair: the chunks' partial tiles added in chunk order.  Written: the entries (a, b) whose 16-column
// tiles are tj <= tk, and their mirror where tj < tk.
__global__ __launch_bounds__(kLanes) void newton_mfma_reduce_kernel(const double* __restrict__ part, int chunks, int ncols,
                                                                     double* __restrict__ M) {
  int tI, tJ;
  macro_pair(blockIdx.x, (ncols + kT - 1) / kT, tI, tJ);
  for (int e = threadIdx.x; e < kT * kT; e += kLanes) {
    const int a = tI * kT + e / kT, b = tJ * kT + e % kT;
    if (a >= ncols || b >= ncols || a / 16 > b / 16) continue;
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += part[((size_t)c * gridDim.x + blockIdx.x) * (size_t)(kT * kT) + e];
    M[(size_t)a * ncols + b] = s;
    if (a / 16 != b / 16) M[(size_t)b * ncols + a] = s;
  }
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
