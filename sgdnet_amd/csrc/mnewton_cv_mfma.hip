// The class-pair moments pass of the wide multinomial Newton cross-validation on the f64 matrix cores (the option
// "cv_wmnewton_moments" = 1; mnewton.hip has the pass it replaces, mnewton_cv_pair_tile_kernel + mnewton_cv_pair_reduce_kernel,
// and says what the moments are).
//
// Job (mix a, training set t) = a * n_sets + t.  For every job whose command of the round is kCvStep and every class pair
// c = (k <= l), over the ncols = p + 2 columns: M_job,c(a, b) = sum_i A(i, a) B_job,c(i, b) over the rows i of the training
// set, with A = [x - m_t | 1 | 0] and B_job,c = [v (x - m_t) | v | r], v(i) = mu_ik (1 - mu_ik) and r(i) = [y_i = k] - mu_ik on
// a diagonal pair, v(i) = -(mu_ik mu_il) and r = 0 otherwise, mu the job's own.  Every term is formed as the old pass forms
// it -- d = x - m rounded, then v d rounded -- and only then multiplied and accumulated by v_mfma_f64_16x16x4_f64; only the
// order of the sum over the rows differs.  ALL n_mix x K (K + 1) / 2 matrices of one training set are Gram matrices of the
// SAME centred rows under another weight per row: mnewton_mfma.hip shares a slab across the class pairs of a fit,
// newton_cv_mfma.hip across the mixes of a set, and this kernel across both.
//
//   members      the members of training set t are the pairs (mix a, class pair c), numbered m = a * class pairs + c.
//   macro tile   as newton_mfma.hip: a workgroup of 256 lanes owns the 64 x 64 entries of one pair of 64-column macro tiles
//                (tI <= tJ; blockIdx.x) over one chunk of the training set's rows (blockIdx.y); wavefront w owns the 32 x 32
//                block (w / 2, w % 2) as 2 x 2 accumulators of 16 x 16; on a diagonal pair the block (1, 0) is left out.
//   group        ... for kG = kWmnewtonCvMfmaGroup consecutive members of ONE training set at once (blockIdx.z = set x groups
//                + group): kG x 2 x 2 accumulators, kG x 16 doubles a lane.  A group may span several mixes, begin in the
//                middle of a mix's class pairs, and the last one may be partial (mnewton.hpp has the cases).
//   taking part  the workgroup reads the commands of its members' jobs first.  A member takes part only if its job's action
//                is kCvStep; for a member that does not step, or that is absent, nothing is issued -- no multiplies, no
//                matrix instructions, no partial tile -- and its matrix stays as it is.  The branch is the same for every
//                lane of the workgroup.  A group with no stepping member, and a chunk beyond the set's chunks, return at once.
//   slab         32 local rows li of the set, global row cv_row(J, li): a slab or a chunk may straddle the gap between the
//                set's two row ranges (each lane maps its own row).  The 64 A columns and the 64 B columns sit in LDS column
//                by column with a stride of 34 doubles, centred once with the set's centres and stored UNWEIGHTED:
//                As[c][i] = d (1.0 in the ones column p, 0.0 in p + 1), Bs[c][i] = d (1.0 in BOTH special columns).  A
//                diagonal pair loads its columns once.  Beside them the slab's weight table Ws[0][g][i] = v, Ws[1][g][i] = r
//                of member g at slab row i, built by lane 32 g + i from that member's job's mu (by local row, a column per
//                class) and y with mnewton_mfma.hip's formulas; 0.0 for rows outside the chunk and for members that do not
//                take part.
//   operands     the A fragments are read from LDS once a slab and serve all members.  So are the B columns' d; for member
//                g a lane forms its B operand in registers as w d, where w is v_g(row) -- or r_g(row) if the lane's column
//                is p + 1: the choice is an LDS address fixed per lane, and v 1.0, r 1.0 are exact, so the special columns
//                cost no branch.  Per slab and member: 16 multiplies and 32 matrix instructions a lane.  The lane layout of
//                the instruction, the rows 8 g .. 8 g + 7 of lane group g and the 16-byte LDS loads are newton_mfma.hip's.
//   overlap      the global loads of slab s + 1 (x, mu_k, mu_l, y) are issued into registers before the matrix instructions
//                of slab s and are centred and stored to LDS after them (one LDS buffer, two barriers a slab).
//   row chunks   a function of (n_t, p, K) alone: wmnewton_mfma_rows_per_chunk(n_t, p + 2, K), what a single fit with
//                "wmnewton_moments" = 1 takes for n_t rows -- never of n_mix or of who steps, so a job's bits do not depend on
//                the other jobs of the call or of its groups.  Every workgroup stores a 64 x 64 partial tile per member that
//                takes part, part[job][class pair][chunk][macro pair]; mnewton_cv_mfma_reduce_kernel adds a stepping job's
//                chunks in chunk order into M[job][class pair]: the 16-column tiles on or above the diagonal, mirrored
//                unless on it -- entry for entry what mnewton_cv_pair_reduce_kernel writes.
// No atomic, and the order of every sum is fixed by (n_t, p, K): the same input gives the same bits.
#include "mnewton_cv_mfma.hpp"

#include "mnewton.hpp"

namespace sgdnet {
namespace {

constexpr int kT = kMfmaTileCols, kS = kMfmaSlabRows, kLanes = 256, kG = kWmnewtonCvMfmaGroup;
constexpr int kStride = kS + 2;                      // doubles between two columns of a slab in LDS
constexpr int kColsPerLane = kT * kS / kLanes;       // 8: the columns of either side a lane stages
static_assert(kT == 64 && kS == 32 && kLanes == 256, "4 wavefronts x (2 x 2) tiles of 16 columns; 4 lane groups x 8 rows");
static_assert(kStride % 2 == 0 && (kStride / 2) % 16 == 1, "16-byte LDS loads: 16 columns fall into 16 different bank groups");
static_assert(kG * kS <= kLanes, "the weight table: lane 32 g + i has member g, row i");

typedef double acc_t __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(kLanes) void mnewton_cv_mfma_tile_kernel(const CvCmd* __restrict__ cmd, const CvJob* __restrict__ jobs,
                                                                       const int64_t* __restrict__ mu_at, const double* __restrict__ x,
                                                                       const double* __restrict__ y, const double* __restrict__ mu_all,
                                                                       const double* __restrict__ m_all, int64_t n, int p, int K,
                                                                       int n_sets, int n_mix, int max_chunks, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) double As[kT][kStride];
  __shared__ __attribute__((aligned(16))) double Bs[kT][kStride];
  __shared__ __attribute__((aligned(16))) double Ws[2][kG][kS];
  const int class_pairs = K * (K + 1) / 2, members = n_mix * class_pairs;
  const int groups = (members + kG - 1) / kG;
  const int set = (int)blockIdx.z / groups, m0 = ((int)blockIdx.z % groups) * kG;       // the group's first member
  unsigned stepping = 0;                             // bit g: member m0 + g is there and its job takes a step in this round
  for (int g = 0; g < kG; ++g)
    if (m0 + g < members && cmd[(size_t)((m0 + g) / class_pairs) * (size_t)n_sets + (size_t)set].action == kCvStep) stepping |= 1u << g;
  if (stepping == 0) return;
  const CvJob J = jobs[set];                         // (the rows and the chunks of a job are its set's: those of mix 0)
  if ((int)blockIdx.y >= J.chunks) return;
  const int tid = threadIdx.x, ncols = p + 2;
  int tI = 0, tJ = 0;
  macro_pair(blockIdx.x, (ncols + kT - 1) / kT, tI, tJ);
  const bool diag = tI == tJ;
  const int64_t r0 = (int64_t)blockIdx.y * J.rows_per_chunk;
  const int64_t r1 = r0 + J.rows_per_chunk < J.n_t ? r0 + J.rows_per_chunk : J.n_t;
  const double* __restrict__ m = m_all + (size_t)set * (size_t)p;

  // staging: row `srow` of the slab, the columns cg + 8 j of either macro tile; and the weights of member cg at that row
  const int srow = tid & (kS - 1), cg = tid / kS;
  double mA[kColsPerLane], mB[kColsPerLane];
  for (int j = 0; j < kColsPerLane; ++j) {
    const int a = tI * kT + cg + 8 * j, b = tJ * kT + cg + 8 * j;
    mA[j] = a < p ? m[a] : 0.0;
    mB[j] = b < p ? m[b] : 0.0;
  }
  const bool weigh = cg < kG && (stepping >> cg & 1u) != 0;
  int ck = 0, cl = 0;
  size_t wjob = 0;
  if (weigh) {
    wjob = (size_t)((m0 + cg) / class_pairs) * (size_t)n_sets + (size_t)set;
    class_pair((m0 + cg) % class_pairs, K, &ck, &cl);
  }
  const double* __restrict__ mu_k = mu_all + mu_at[wjob] + (int64_t)ck * J.n_t;      // (by the job's local row)
  const double* __restrict__ mu_l = mu_all + mu_at[wjob] + (int64_t)cl * J.n_t;
  double xa[kColsPerLane], xb[kColsPerLane], pk = 0.0, pl = 0.0, yi = 0.0;
  bool live = false;
  auto load = [&](int64_t base) {          // the slab's values into registers; nothing outside the chunk, the set or x is read
    const int64_t li = base + srow;
    live = li < r1;
    const int64_t i = live ? cv_row(J, li) : 0;
    pk = weigh && live ? mu_k[li] : 0.0;
    pl = weigh && live ? mu_l[li] : 0.0;
    yi = weigh && live ? y[i] : 0.0;
#pragma unroll
    for (int j = 0; j < kColsPerLane; ++j) {
      const int a = tI * kT + cg + 8 * j, b = tJ * kT + cg + 8 * j;
      xa[j] = live && a < p ? x[i + (int64_t)a * n] : 0.0;
      xb[j] = !diag && live && b < p ? x[i + (int64_t)b * n] : 0.0;
    }
  };
  auto store = [&]() {                     // centred as mnewton_cv_pair_tile_kernel centres them; the weights as it forms them
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
        if ((stepping >> g & 1u) == 0) continue;       // (the same for every lane of the workgroup)
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
  // part[job][class pair][chunk][macro pair][64 x 64]
#pragma unroll
  for (int g = 0; g < kG; ++g) {
    if ((stepping >> g & 1u) == 0) continue;
    const size_t job = (size_t)((m0 + g) / class_pairs) * (size_t)n_sets + (size_t)set, cp = (size_t)((m0 + g) % class_pairs);
    double* out = part + (((job * (size_t)class_pairs + cp) * (size_t)max_chunks + blockIdx.y) * gridDim.x + blockIdx.x) * (size_t)(kT * kT);
#pragma unroll
    for (int ta = 0; ta < 2; ++ta)
#pragma unroll
      for (int tb = 0; tb < 2; ++tb)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          out[(wa * 32 + ta * 16 + 4 * e + lg) * kT + wb * 32 + tb * 16 + lc] = acc[g][ta][tb][e];
  }
}

// blockIdx.x = macro-tile pair, blockIdx.y = job x class pairs + class pair: a stepping job's partial tiles added in chunk
// order into M[job][class pair].  Written: the entries (a, b) whose 16-column tiles are tj <= tk, and their mirror where tj < tk.
__global__ __launch_bounds__(kLanes) void mnewton_cv_mfma_reduce_kernel(const CvCmd* __restrict__ cmd, const CvJob* __restrict__ jobs,
                                                                         const double* __restrict__ part, int class_pairs, int max_chunks,
                                                                         int ncols, double* __restrict__ M_all) {
  const int job = (int)blockIdx.y / class_pairs;
  if (cmd[job].action != kCvStep) return;
  int tI = 0, tJ = 0;
  macro_pair(blockIdx.x, (ncols + kT - 1) / kT, tI, tJ);
  const int chunks = jobs[job].chunks;
  double* __restrict__ M = M_all + (size_t)blockIdx.y * (size_t)ncols * (size_t)ncols;
  for (int e = threadIdx.x; e < kT * kT; e += kLanes) {
    const int a = tI * kT + e / kT, b = tJ * kT + e % kT;
    if (a >= ncols || b >= ncols || a / 16 > b / 16) continue;
    double s = 0.0;
    for (int c = 0; c < chunks; ++c)
      s += part[(((size_t)blockIdx.y * (size_t)max_chunks + c) * gridDim.x + blockIdx.x) * (size_t)(kT * kT) + e];
    M[(size_t)a * ncols + b] = s;
    if (a / 16 != b / 16) M[(size_t)b * ncols + a] = s;
  }
}

}  // namespace

void wmnewton_cv_mfma_moments(const CvCmd* cmd, const CvJob* jobs, const int64_t* mu_at, const double* x, const double* y,
                              const double* mu_all, const double* m_all, int64_t n, int p, int K, int n_sets, int n_mix, int max_chunks,
                              double* part, double* M_all, hipStream_t st) {
  const int ncols = p + 2, class_pairs = K * (K + 1) / 2;
  const unsigned pairs = (unsigned)wide_mfma_pairs(ncols), groups = (unsigned)wmnewton_cv_mfma_groups(n_mix, K);
  hipLaunchKernelGGL(mnewton_cv_mfma_tile_kernel, dim3(pairs, (unsigned)max_chunks, (unsigned)n_sets * groups), dim3(kLanes), 0, st, cmd, jobs,
                     mu_at, x, y, mu_all, m_all, n, p, K, n_sets, n_mix, max_chunks, part);
  hipLaunchKernelGGL(mnewton_cv_mfma_reduce_kernel, dim3(pairs, (unsigned)n_sets * (unsigned)n_mix * (unsigned)class_pairs), dim3(kLanes), 0, st,
                     cmd, jobs, part, class_pairs, max_chunks, ncols, M_all);
}

}  // namespace sgdnet
