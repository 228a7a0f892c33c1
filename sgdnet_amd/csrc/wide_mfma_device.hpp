// The slab/tile core the f64 matrix-core moments passes of the wide Newton modes share (newton_mfma.hip, mnewton_mfma.hip,
// newton_cv_mfma.hip, mnewton_cv_mfma.hip).  Included by those four units only (HIP types in here; never by fit_plan.hpp);
// everything has internal linkage (each unit gets its own copy, as if it were written in it).  The geometry constants and
// the row chunks are wide_layout.hpp's.
//
// M(a, b) = sum_i A(i, a) B(i, b) over the ncols = p + 2 columns A = [x - mu | 1 | 0], B = [w (x - mu) | w | r] for a weight w
// and a residual r per row.  Every term is formed as the passes these replace form it -- d = x - mu rounded, then w d
// rounded -- and only then multiplied and accumulated by v_mfma_f64_16x16x4_f64 (a fused multiply-add per term); only the
// order of the sum over the rows differs.
//
//   macro tile   a workgroup of 256 lanes (4 wavefronts) owns the 64 x 64 entries (a, b) of one pair of 64-column macro
//                tiles (tI <= tJ; blockIdx.x) over one chunk of rows (blockIdx.y); wavefront w owns the 32 x 32 block
//                (w / 2, w % 2) of it as 2 x 2 accumulators of 16 x 16: 4 x 4 doubles a lane.  On a diagonal pair the
//                block (1, 0) lies below the diagonal 16-column tiles and is left out.
//   slab         32 rows of the 64 A columns and the 64 B columns, staged in LDS column by column with a stride of 34
//                doubles: As[c][i] = A(i, c), Bs[c][i] = B(i, c), centred once, as they are stored.  x is column-major:
//                lane t loads row t % 32 of the columns t / 32 + 8 j, 32 consecutive doubles a column.  A diagonal pair
//                loads its columns once and stores both forms.
//   operands     the instruction multiplies a 16 x 4 by a 4 x 16 block: lane l supplies A[l % 16][l / 16] and
//                B[l / 16][l % 16] and holds D[4 e + l / 16][l % 16] in element e of its accumulator.  The order of the
//                rows within a slab is free as long as A and B agree, so lane group g = l / 16 takes the rows 8 g .. 8 g + 7
//                in the slab's 8 steps: a lane reads its 8 rows of a column as four 16-byte LDS loads.  Stride 34: the 16
//                lanes of a group read 16 columns 272 bytes apart, 17 x 16 bytes: every 16-byte bank group once.
//   overlap      the global loads of slab s + 1 are issued into registers before the 32 matrix instructions of slab s and
//                are centred and stored to LDS after them (one LDS buffer, two barriers a slab).
//   row chunks   every workgroup stores its 64 x 64 partial tile, and the unit's reduce kernel adds the chunks in chunk
//                order into M: the 16-column tiles on or above the diagonal, mirrored unless on it (a diagonal 16-column
//                tile holds both of its triangles as computed: M(p + 1, .) = 0 there, M(., p + 1) = q).
//   group        the matrices of one set of rows under several weights (the class pairs of a fit, the mixes of a training
//                set) are Gram matrices of the SAME centred rows, so a workgroup of mfma_group_tile serves kG members at
//                once: kG x 2 x 2 accumulators, kG x 16 doubles a lane.  The slab is stored UNWEIGHTED -- Bs[c][i] = d, 1.0
//                in BOTH special columns -- beside the weight table Ws[0][g][i] = w, Ws[1][g][i] = r of member g at slab
//                row i, written by lane 32 g + i; 0.0 for rows outside the chunk and for members that take no part.  The
//                A fragments and the B columns' d are read from LDS once a slab and serve all members; for member g a
//                lane forms its B operand in registers as w d, or r d if the lane's column is p + 1: the choice is an LDS
//                address fixed per lane, and w 1.0, r 1.0 are exact, so the special columns cost no branch.  Per slab and
//                member: 16 multiplies and 32 matrix instructions a lane.  For a member that takes no part nothing is
//                issued -- no multiplies, no matrix instructions, no partial tile; the branch is the same for every lane.
// No atomic, and the order of every sum is fixed by the shape: the same input gives the same bits.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wide_layout.hpp"

namespace sgdnet {
namespace {

constexpr int kT = kMfmaTileCols, kS = kMfmaSlabRows, kLanes = 256;
constexpr int kStride = kS + 2;                      // doubles between two columns of a slab in LDS
constexpr int kColsPerLane = kT * kS / kLanes;       // 8: the columns of either side a lane stages
static_assert(kT == 64 && kS == 32 && kLanes == 256, "4 wavefronts x (2 x 2) tiles of 16 columns; 4 lane groups x 8 rows");
static_assert(kStride % 2 == 0 && (kStride / 2) % 16 == 1, "16-byte LDS loads: 16 columns fall into 16 different bank groups");

typedef double acc_t __attribute__((ext_vector_type(4)));
typedef double slab_t[kT][kStride];                  // one side of a slab in LDS (declare it aligned(16))

// A lane's place in its workgroup's macro-tile pair (blockIdx.x) and row chunk (blockIdx.y): the local rows [r0, r1)
struct MfmaTile {
  int tI, tJ;
  bool diag;
  int64_t r0, r1;
  int srow, cg;            // staging: row `srow` of the slab, the columns cg + 8 j of either macro tile
  int wa, wb, lc, lg;      // the matrix instructions: lane group lg takes the rows 8 lg .. 8 lg + 7 of the slab, column lc
  bool idle;               //   of each 16-column tile of the block (wa, wb); idle: below the diagonal 16-column tiles
  __device__ MfmaTile(int ncols, int64_t rows_per_chunk, int64_t rows) {
    macro_pair(blockIdx.x, (ncols + kT - 1) / kT, tI, tJ);
    diag = tI == tJ;
    r0 = (int64_t)blockIdx.y * rows_per_chunk;
    r1 = r0 + rows_per_chunk < rows ? r0 + rows_per_chunk : rows;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    srow = tid & (kS - 1), cg = tid / kS;
    lc = lane & 15, lg = lane >> 4, wa = wave >> 1, wb = wave & 1;
    idle = diag && wa > wb;
  }
};

// The x part of a lane's staging: its columns' centres, and a slab's values in registers between load and store
struct MfmaColumns {
  double muA[kColsPerLane], muB[kColsPerLane], xa[kColsPerLane], xb[kColsPerLane];
  bool live = false;
  __device__ MfmaColumns(const MfmaTile& L, const double* __restrict__ mu, int p) {
    for (int j = 0; j < kColsPerLane; ++j) {
      const int a = L.tI * kT + L.cg + 8 * j, b = L.tJ * kT + L.cg + 8 * j;
      muA[j] = a < p ? mu[a] : 0.0;
      muB[j] = b < p ? mu[b] : 0.0;
    }
  }
  // row i of x (column-major, n rows) if the lane's slab row is `in_chunk`; nothing outside the chunk or x is read
  __device__ __forceinline__ void load(const MfmaTile& L, const double* __restrict__ x, int64_t n, int p, int64_t i, bool in_chunk) {
    live = in_chunk;
#pragma unroll
    for (int j = 0; j < kColsPerLane; ++j) {
      const int a = L.tI * kT + L.cg + 8 * j, b = L.tJ * kT + L.cg + 8 * j;
      xa[j] = live && a < p ? x[i + (int64_t)a * n] : 0.0;
      xb[j] = !L.diag && live && b < p ? x[i + (int64_t)b * n] : 0.0;
    }
  }
  // centred as the dense tile kernels centre them: As = d, 1.0 in the ones column p; Bs = b_of(column b, d), d = 1.0 in
  // both special columns
  template <class BOf>
  __device__ __forceinline__ void store(const MfmaTile& L, slab_t As, slab_t Bs, int p, BOf b_of) const {
#pragma unroll
    for (int j = 0; j < kColsPerLane; ++j) {
      const int c = L.cg + 8 * j, a = L.tI * kT + c, b = L.tJ * kT + c;
      const double da = a < p ? xa[j] - muA[j] : (a == p ? 1.0 : 0.0);
      const double db = b < p ? (L.diag ? xa[j] : xb[j]) - muB[j] : (b <= p + 1 ? 1.0 : 0.0);
      As[c][L.srow] = live ? da : 0.0;
      Bs[c][L.srow] = live ? b_of(b, db) : 0.0;
    }
  }
};

// The pipeline of a chunk: load(base) takes the slab of the local rows base .. base + 31 into registers, store() puts the
// loaded slab into LDS, compute() is a busy lane's work on the stored slab
template <class Load, class Store, class Compute>
__device__ __forceinline__ void mfma_slabs(const MfmaTile& L, Load load, Store store, Compute compute) {
  load(L.r0);
  for (int64_t base = L.r0; base < L.r1; base += kS) {
    store();
    __syncthreads();
    if (base + kS < L.r1) load(base + kS);
    if (!L.idle) compute();
    __syncthreads();
  }
}

// a lane's 8 rows of its two A columns and its two B columns
__device__ __forceinline__ void mfma_fragments(const MfmaTile& L, const slab_t As, const slab_t Bs, double fa[2][8], double fb[2][8]) {
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const double2* pa = reinterpret_cast<const double2*>(&As[L.wa * 32 + t * 16 + L.lc][L.lg * 8]);
    const double2* pb = reinterpret_cast<const double2*>(&Bs[L.wb * 32 + t * 16 + L.lc][L.lg * 8]);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const double2 qa = pa[s], qb = pb[s];
      fa[t][2 * s] = qa.x;
      fa[t][2 * s + 1] = qa.y;
      fb[t][2 * s] = qb.x;
      fb[t][2 * s + 1] = qb.y;
    }
  }
}

// the slab's 8 steps into the 2 x 2 accumulators
__device__ __forceinline__ void mfma_block(const double fa[2][8], const double fb[2][8], acc_t acc[2][2]) {
#pragma unroll
  for (int s = 0; s < 8; ++s)
#pragma unroll
    for (int ta = 0; ta < 2; ++ta)
#pragma unroll
      for (int tb = 0; tb < 2; ++tb) acc[ta][tb] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[ta][s], fb[tb][s], acc[ta][tb], 0, 0, 0);
}

// a busy lane's 2 x 2 x 4 entries into the 64 x 64 partial tile `out`
__device__ __forceinline__ void mfma_store_tile(const MfmaTile& L, double* __restrict__ out, const acc_t acc[2][2]) {
#pragma unroll
  for (int ta = 0; ta < 2; ++ta)
#pragma unroll
    for (int tb = 0; tb < 2; ++tb)
#pragma unroll
      for (int e = 0; e < 4; ++e) out[(L.wa * 32 + ta * 16 + 4 * e + L.lg) * kT + L.wb * 32 + tb * 16 + L.lc] = acc[ta][tb][e];
}

// The body of a reduce kernel (blockIdx.x = macro-tile pair).  first: the partial tile of the matrix's chunk 0 and this
// pair; stride: the doubles between the tiles of two chunks.  Written: the entries (a, b) of M whose 16-column tiles are
// tj <= tk, and their mirror where tj < tk.
__device__ __forceinline__ void mfma_reduce(const double* __restrict__ first, size_t stride, int chunks, int ncols, double* __restrict__ M) {
  int tI = 0, tJ = 0;
  macro_pair(blockIdx.x, (ncols + kT - 1) / kT, tI, tJ);
  for (int e = threadIdx.x; e < kT * kT; e += kLanes) {
    const int a = tI * kT + e / kT, b = tJ * kT + e % kT;
    if (a >= ncols || b >= ncols || a / 16 > b / 16) continue;
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += first[(size_t)c * stride + e];
    M[(size_t)a * ncols + b] = s;
    if (a / 16 != b / 16) M[(size_t)b * ncols + a] = s;
  }
}

// The tile kernel's body for a group of kG members over the rows of L.  x: column-major with n rows; mu: the p centres.
// What a unit states of its own is G (all but the weights the same for every lane of the workgroup):
//   bool G.member(g)                  does member g < kG take part
//   int64_t G.row(li, live)           the row of x and y that is local row li (live: li is in the chunk; else not read)
//   G.load(li, i, live)               the lane's weight source at that row into registers: lane (cg, srow) has member cg
//   G.weights(live, v, r)             ... and from them the member's w and r there; 0.0 unless live and the member takes part
//   double* G.tile(g)                 member g's 64 x 64 partial tile of this workgroup
template <int kG, class Group>
__device__ __forceinline__ void mfma_group_tile(const MfmaTile& L, Group& G, const double* __restrict__ x, const double* __restrict__ mu,
                                                int64_t n, int p) {
  static_assert(kG * kS <= kLanes, "the weight table: lane 32 g + i has member g, row i");
  __shared__ __attribute__((aligned(16))) slab_t As;
  __shared__ __attribute__((aligned(16))) slab_t Bs;
  __shared__ __attribute__((aligned(16))) double Ws[2][kG][kS];
  MfmaColumns X(L, mu, p);
  auto load = [&](int64_t base) {
    const int64_t li = base + L.srow;
    const bool live = li < L.r1;
    const int64_t i = G.row(li, live);
    G.load(li, i, live);
    X.load(L, x, n, p, i, live);
  };
  auto store = [&]() {
    X.store(L, As, Bs, p, [](int, double d) { return d; });
    if (L.cg < kG) {
      double w, r;
      G.weights(X.live, w, r);
      Ws[0][L.cg][L.srow] = w;
      Ws[1][L.cg][L.srow] = r;
    }
  };
  int wsel[2];                             // which weight the lane's B column takes: r in column p + 1, w elsewhere
  for (int t = 0; t < 2; ++t) wsel[t] = L.tJ * kT + L.wb * 32 + t * 16 + L.lc == p + 1 ? 1 : 0;
  acc_t acc[kG][2][2];
#pragma unroll
  for (int g = 0; g < kG; ++g)
    for (int ta = 0; ta < 2; ++ta)
      for (int tb = 0; tb < 2; ++tb) acc[g][ta][tb] = acc_t{0.0, 0.0, 0.0, 0.0};

  mfma_slabs(L, load, store, [&]() {
    double fa[2][8], fd[2][8];
    mfma_fragments(L, As, Bs, fa, fd);
#pragma unroll
    for (int g = 0; g < kG; ++g) {
      if (!G.member(g)) continue;
      double fb[2][8];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const double2* pw = reinterpret_cast<const double2*>(&Ws[wsel[t]][g][L.lg * 8]);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const double2 qw = pw[s];
          fb[t][2 * s] = qw.x * fd[t][2 * s];
          fb[t][2 * s + 1] = qw.y * fd[t][2 * s + 1];
        }
      }
      mfma_block(fa, fb, acc[g]);
    }
  });
  if (L.idle) return;
#pragma unroll
  for (int g = 0; g < kG; ++g)
    if (G.member(g)) mfma_store_tile(L, G.tile(g), acc[g]);
}

// The weight source of the multinomial units: the lane's member is class pair (ck <= cl) of a fit whose mu_k, mu_l are read
// by local row and y by row of x.  v = mu_k (1 - mu_k) and r = [y = k] - mu_k on a diagonal pair, v = -(mu_k mu_l) and
// r = 0 otherwise, as mnewton_pair_tile_kernel forms them.  weigh: the lane has a member and it takes part.
struct ClassPairWeights {
  bool weigh;
  int ck, cl;
  const double *mu_k, *mu_l, *y;
  double pk = 0.0, pl = 0.0, yi = 0.0;
  __device__ __forceinline__ void load(int64_t li, int64_t i, bool live) {
    pk = weigh && live ? mu_k[li] : 0.0;
    pl = weigh && live ? mu_l[li] : 0.0;
    yi = weigh && live ? y[i] : 0.0;
  }
  __device__ __forceinline__ void weights(bool live, double& v, double& r) const {
    v = r = 0.0;
    if (!(weigh && live)) return;
    if (ck == cl) {
      v = pk * (1.0 - pk);
      r = ((int)(yi + 0.5) == ck ? 1.0 : 0.0) - pk;
    } else {
      v = -(pk * pl);
    }
  }
};

}  // namespace
}  // namespace sgdnet
