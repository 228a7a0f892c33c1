// The class-pair moments pass of wide multinomial Newton mode on the f64 matrix cores (the option "wmnewton_moments" = 1;
// mnewton.hip has the pass it replaces, mnewton_pair_tile_kernel + mnewton_pair_reduce_kernel, and says what the moments are).
//
// For every class pair c = (k <= l), over the ncols = p + 2 columns: M_c(a, b) = sum_i A(i, a) B_c(i, b) with
// A = [x - m | 1 | 0] and B_c = [v_c (x - m) | v_c | r_c], v_c(i) = mu_ik (1 - mu_ik) and r_c(i) = [y_i = k] - mu_ik on a
// diagonal pair, v_c(i) = -(mu_ik mu_il) and r_c = 0 otherwise.  Every term is formed as the old pass forms it -- d = x - m
// rounded, then v d rounded -- and only then multiplied and accumulated by v_mfma_f64_16x16x4_f64; only the order of the
// sum over the rows differs.  All K (K + 1) / 2 matrices are Gram matrices of the SAME centred rows under another weight
// per row, and the kernel is built around that: what is loaded, centred and staged is shared by a group of class pairs.
//
//   macro tile   as newton_mfma.hip: a workgroup of 256 lanes owns the 64 x 64 entries of one pair of 64-column macro tiles
//                (tI <= tJ; blockIdx.x) over one chunk of rows (blockIdx.y); wavefront w owns the 32 x 32 block (w / 2, w % 2)
//                as 2 x 2 accumulators of 16 x 16; on a diagonal pair the block (1, 0) is left out.
//   group        ... for kG = kWmnewtonMfmaGroup consecutive class pairs at once (blockIdx.z): kG x 2 x 2 accumulators,
//                kG x 16 doubles a lane.  The last group of a K may be partial; its absent pairs issue nothing.
//   slab         32 rows of the 64 A columns and the 64 B columns in LDS, column by column with a stride of 34 doubles,
//                centred once and stored UNWEIGHTED: As[c][i] = d (1.0 in the ones column p, 0.0 in p + 1), Bs[c][i] = d (1.0
//                in BOTH special columns).  Beside them the slab's weight table Ws[0][g][i] = v_g(i), Ws[1][g][i] = r_g(i),
//                built from mu and y by lane 32 g + i; 0.0 for rows outside the chunk and for absent pairs.
//   operands     the A fragments are read from LDS once a slab and serve all kG pairs.  So are the B columns' d; for pair
//                g a lane forms its B operand in registers as w d, where w is v_g(row) -- or r_g(row) if the lane's column
//                is p + 1: the choice is an LDS address fixed per lane, and v 1.0, r 1.0 are exact, so the special columns
//                cost no branch.  Per slab and pair: 16 multiplies and 32 matrix instructions a lane.  The lane layout of
//                the instruction, the rows 8 g .. 8 g + 7 of lane group g and the 16-byte LDS loads are newton_mfma.hip's.
//   overlap      the global loads of slab s + 1 (x, the mu of the lane's class pair, y) are issued into registers before
//                the matrix instructions of slab s and are centred and stored to LDS after them.
//   row chunks   mnewton.hpp: wmnewton_mfma_rows_per_chunk, over macro pairs x groups workgroups a chunk.  Every workgroup
//                stores a 64 x 64 partial tile per class pair of its group; mnewton_mfma_reduce_kernel adds the chunks in
//                chunk order into each pair's matrix: the 16-column tiles on or above the diagonal, mirrored unless on it --
//                entry for entry what mnewton_pair_reduce_kernel writes.
// No atomic, and the order of every sum is fixed by (n, p, K): the same input gives the same bits.
#include "mnewton_mfma.hpp"

#include "mnewton.hpp"

namespace sgdnet {
namespace {

constexpr int kT = kMfmaTileCols, kS = kMfmaSlabRows, kLanes = 256, kG = kWmnewtonMfmaGroup;
constexpr int kStride = kS + 2;                      // doubles between two columns of a slab in LDS
constexpr int kColsPerLane = kT * kS / kLanes;       // 8: the columns of either side a lane stages
static_assert(kT == 64 && kS == 32 && kLanes == 256, "4 wavefronts x (2 x 2) tiles of 16 columns; 4 lane groups x 8 rows");
static_assert(kStride % 2 == 0 && (kStride / 2) % 16 == 1, "16-byte LDS loads: 16 columns fall into 16 different bank groups");
static_assert(kG * kS <= kLanes, "the weight table: lane 32 g + i has pair g, row i");

typedef double acc_t __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(kLanes) void mnewton_mfma_tile_kernel(const double* __restrict__ x, const double* __restrict__ y,
                                                                    const double* __restrict__ mu, const double* __restrict__ m, int64_t n,
                                                                    int p, int K, int64_t rows_per_chunk, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) double As[kT][kStride];
  __shared__ __attribute__((aligned(16))) double Bs[kT][kStride];
  __shared__ __attribute__((aligned(16))) double Ws[2][kG][kS];
  const int tid = threadIdx.x, ncols = p + 2, class_pairs = K * (K + 1) / 2;
  int tI = 0, tJ = 0;
  macro_pair(blockIdx.x, (ncols + kT - 1) / kT, tI, tJ);
  const bool diag = tI == tJ;
  const int c0 = (int)blockIdx.z * kG;                                   // the group's first class pair
  const int present = class_pairs - c0 < kG ? class_pairs - c0 : kG;     // ... and how many it has
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_chunk;
  const int64_t r1 = r0 + rows_per_chunk < n ? r0 + rows_per_chunk : n;

  // staging: row `srow` of the slab, the columns cg + 8 j of either macro tile; and the weights of pair cg at that row
  const int srow = tid & (kS - 1), cg = tid / kS;
  double mA[kColsPerLane], mB[kColsPerLane];
  for (int j = 0; j < kColsPerLane; ++j) {
    const int a = tI * kT + cg + 8 * j, b = tJ * kT + cg + 8 * j;
    mA[j] = a < p ? m[a] : 0.0;
    mB[j] = b < p ? m[b] : 0.0;
  }
  const bool weigh = cg < present;
  int ck = 0, cl = 0;
  if (weigh) class_pair(c0 + cg, K, &ck, &cl);
  const double* __restrict__ mu_k = mu + (int64_t)ck * n;
  const double* __restrict__ mu_l = mu + (int64_t)cl * n;
  double xa[kColsPerLane], xb[kColsPerLane], pk = 0.0, pl = 0.0, yi = 0.0;
  bool live = false;
  auto load = [&](int64_t base) {          // the slab's values into registers; nothing outside the chunk, x or mu is read
    const int64_t i = base + srow;
    live = i < r1;
    pk = weigh && live ? mu_k[i] : 0.0;
    pl = weigh && live ? mu_l[i] : 0.0;
    yi = weigh && live ? y[i] : 0.0;
#pragma unroll
    for (int j = 0; j < kColsPerLane; ++j) {
      const int a = tI * kT + cg + 8 * j, b = tJ * kT + cg + 8 * j;
      xa[j] = live && a < p ? x[i + (int64_t)a * n] : 0.0;
      xb[j] = !diag && live && b < p ? x[i + (int64_t)b * n] : 0.0;
    }
  };
  auto store = [&]() {                     // centred as mnewton_pair_tile_kernel centres them; the weights as it forms them
#pragma unroll
    for (int j = 0; j < kColsPerLane; ++j) {
      const int c = cg + 8 * j, a = tI * kT + c, b = tJ * kT + c;
      const double da = a < p ? xa[j] - mA[j] : (a == p ? 1.0 : 0.0);
      const double db = b < p ? (diag ? xa[j] : xb[j]) - mB[j] : (b <= p + 1 ? 1.0 : 0.0);
      As[c][srow] = live ? da : 0.0;
      Bs[c][srow] = live ? db : 0.0;
    }
    if (cg < kG) {
      double v = 0.0, r = 0.0;
      if (weigh && live) {
        if (ck == cl) {
          v = pk * (1.0 - pk);
          r = ((int)(yi + 0.5) == ck ? 1.0 : 0.0) - pk;
        } else {
          v = -(pk * pl);
        }
      }
      Ws[0][cg][srow] = v;
      Ws[1][cg][srow] = r;
    }
  };

  // the matrix instructions: lane group g takes the rows 8 g .. 8 g + 7 of the slab, column l % 16 of each 16-column tile
  const int wave = tid >> 6, lane = tid & 63, lc = lane & 15, lg = lane >> 4;
  const int wa = wave >> 1, wb = wave & 1;
  const bool idle = diag && wa > wb;       // below the diagonal 16-column tiles
  int wsel[2];                             // which weight the lane's B column takes: r in column p + 1, v elsewhere
  for (int t = 0; t < 2; ++t) wsel[t] = tJ * kT + wb * 32 + t * 16 + lc == p + 1 ? 1 : 0;
  acc_t acc[kG][2][2];
#pragma unroll
  for (int g = 0; g < kG; ++g)
    for (int ta = 0; ta < 2; ++ta)
      for (int tb = 0; tb < 2; ++tb) acc[g][ta][tb] = acc_t{0.0, 0.0, 0.0, 0.0};

  load(r0);
  for (int64_t base = r0; base < r1; base += kS) {
    store();
    __syncthreads();
    if (base + kS < r1) load(base + kS);
    if (!idle) {
      double fa[2][8], fd[2][8];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const double2* pa = reinterpret_cast<const double2*>(&As[wa * 32 + t * 16 + lc][lg * 8]);
        const double2* pd = reinterpret_cast<const double2*>(&Bs[wb * 32 + t * 16 + lc][lg * 8]);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const double2 qa = pa[s], qd = pd[s];
          fa[t][2 * s] = qa.x;
          fa[t][2 * s + 1] = qa.y;
          fd[t][2 * s] = qd.x;
          fd[t][2 * s + 1] = qd.y;
        }
      }
#pragma unroll
      for (int g = 0; g < kG; ++g) {
        if (g >= present) break;           // (the same for every lane of the workgroup)
        double fb[2][8];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const double2* pw = reinterpret_cast<const double2*>(&Ws[wsel[t]][g][lg * 8]);
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const double2 qw = pw[s];
            fb[t][2 * s] = qw.x * fd[t][2 * s];
            fb[t][2 * s + 1] = qw.y * fd[t][2 * s + 1];
          }
        }
#pragma unroll
        for (int s = 0; s < 8; ++s)
#pragma unroll
          for (int ta = 0; ta < 2; ++ta)
#pragma unroll
            for (int tb = 0; tb < 2; ++tb)
              acc[g][ta][tb] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[ta][s], fb[tb][s], acc[g][ta][tb], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  if (idle) return;
  // part[chunk][class pair][macro pair][64 x 64]
#pragma unroll
  for (int g = 0; g < kG; ++g) {
    if (g >= present) break;
    double* out = part + (((size_t)blockIdx.y * (size_t)class_pairs + (size_t)(c0 + g)) * gridDim.x + blockIdx.x) * (size_t)(kT * kT);
#pragma unroll
    for (int ta = 0; ta < 2; ++ta)
#pragma unroll
      for (int tb = 0; tb < 2; ++tb)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          out[(wa * 32 + ta * 16 + 4 * e + lg) * kT + wb * 32 + tb * 16 + lc] = acc[g][ta][tb][e];
  }
}

// blockIdx.x = macro-tile pair, blockIdx.y = class pair: the chunks' partial tiles added in chunk order into M[class pair].
// Written: the entries (a, b) whose 16-column tiles are tj <= tk, and their mirror where tj < tk.
__global__ __launch_bounds__(kLanes) void mnewton_mfma_reduce_kernel(const double* __restrict__ part, int chunks, int ncols,
                                                                      double* __restrict__ M_all) {
  int tI = 0, tJ = 0;
  macro_pair(blockIdx.x, (ncols + kT - 1) / kT, tI, tJ);
  double* __restrict__ M = M_all + (size_t)blockIdx.y * (size_t)ncols * (size_t)ncols;
  for (int e = threadIdx.x; e < kT * kT; e += kLanes) {
    const int a = tI * kT + e / kT, b = tJ * kT + e % kT;
    if (a >= ncols || b >= ncols || a / 16 > b / 16) continue;
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += part[(((size_t)c * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * (size_t)(kT * kT) + e];
    M[(size_t)a * ncols + b] = s;
    if (a / 16 != b / 16) M[(size_t)b * ncols + a] = s;
  }
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
