// The class-pair moments pass of the wide multinomial Newton cross-validation on the f64 matrix cores (the option
// "cv_wmnewton_moments" = 1; mnewton.hip has the pass it replaces, mnewton_cv_pair_tile_kernel + mnewton_cv_pair_reduce_kernel,
// and says what the moments are).
//
// Job (mix a, training set t) = a * n_sets + t.  For every job whose command of the round is kCvStep and every class pair
// c = (k <= l): M_job,c(a, b) = sum_i A(i, a) B_job,c(i, b) over the rows i of the training set, with A = [x - m_t | 1 | 0] and
// B_job,c = [v (x - m_t) | v | r], v and r of the job's own mu.  ALL n_mix x K (K + 1) / 2 matrices of one training set are
// Gram matrices of the SAME centred rows under another weight per row: mnewton_mfma.hip shares a slab across the class pairs
// of a fit, newton_cv_mfma.hip across the mixes of a set, and this kernel across both.  It is the grouped tile of
// wide_mfma_device.hpp, which has the geometry.  This unit's own:
//   rows         as newton_cv_mfma.hip: local row li of the set is row cv_row(J, li).  The chunks are a function of
//                (n_t, p, K) alone: wmnewton_mfma_rows_per_chunk(n_t, p + 2, K), what a single fit with "wmnewton_moments" = 1
//                takes for n_t rows -- never of n_mix or of who steps, so a job's bits do not depend on the other jobs of the
//                call or of its groups.  A chunk beyond the set's chunks returns at once.
//   weights      formed from the member's job's mu (by local row, a column per class) and y (ClassPairWeights)
//   members      the members of training set t are the pairs (mix a, class pair c), numbered m = a * class pairs + c;
//                kG = kWmnewtonCvMfmaGroup consecutive ones of ONE training set (blockIdx.z = set x groups + group).  A group
//                may span several mixes, begin in the middle of a mix's class pairs, and the last one may be partial
//                (mnewton.hpp has the cases).  The workgroup reads the commands of its members' jobs first: a member takes
//                part only if its job's action is kCvStep; the matrix of one that does not step, or is absent, stays as it
//                is.  A group with no stepping member returns at once.
//   tiles        part[job][class pair][chunk][macro pair]; the reduce kernel adds a stepping job's chunks into
//                M[job][class pair], entry for entry what mnewton_cv_pair_reduce_kernel writes
#include "mnewton_cv_mfma.hpp"

#include "mnewton.hpp"
#include "wide_mfma_device.hpp"

namespace sgdnet {
namespace {

constexpr int kG = kWmnewtonCvMfmaGroup;

struct SetClassPairs : ClassPairWeights {
  CvJob J;                               // (the rows and the chunks of a job are its set's: those of mix 0)
  unsigned stepping;                     // bit g: member m0 + g is there and its job takes a step in this round
  int m0, class_pairs, set, n_sets, max_chunks;
  double* part;
  __device__ bool member(int g) const { return (stepping >> g & 1u) != 0; }
  __device__ size_t job(int g) const { return (size_t)((m0 + g) / class_pairs) * (size_t)n_sets + (size_t)set; }
  __device__ int64_t row(int64_t li, bool live) const { return live ? cv_row(J, li) : 0; }
  __device__ double* tile(int g) const {
    const size_t cp = (size_t)((m0 + g) % class_pairs);
    return part + (((job(g) * (size_t)class_pairs + cp) * (size_t)max_chunks + blockIdx.y) * gridDim.x + blockIdx.x) * (size_t)(kT * kT);
  }
};

__global__ __launch_bounds__(kLanes) void mnewton_cv_mfma_tile_kernel(const CvCmd* __restrict__ cmd, const CvJob* __restrict__ jobs,
                                                                       const int64_t* __restrict__ mu_at, const double* __restrict__ x,
                                                                       const double* __restrict__ y, const double* __restrict__ mu_all,
                                                                       const double* __restrict__ m_all, int64_t n, int p, int K,
                                                                       int n_sets, int n_mix, int max_chunks, double* __restrict__ part) {
  const int class_pairs = K * (K + 1) / 2, members = n_mix * class_pairs;
  const int groups = (members + kG - 1) / kG;
  const int set = (int)blockIdx.z / groups, m0 = ((int)blockIdx.z % groups) * kG;       // the group's first member
  unsigned stepping = 0;
  for (int g = 0; g < kG; ++g)
    if (m0 + g < members && cmd[(size_t)((m0 + g) / class_pairs) * (size_t)n_sets + (size_t)set].action == kCvStep) stepping |= 1u << g;
  if (stepping == 0) return;
  SetClassPairs G;
  G.J = jobs[set];
  if ((int)blockIdx.y >= G.J.chunks) return;
  G.stepping = stepping, G.m0 = m0, G.class_pairs = class_pairs, G.set = set, G.n_sets = n_sets, G.max_chunks = max_chunks, G.part = part;
  const MfmaTile L(p + 2, G.J.rows_per_chunk, G.J.n_t);
  G.weigh = L.cg < kG && G.member(L.cg);
  G.ck = G.cl = 0;
  size_t wjob = 0;
  if (G.weigh) {
    wjob = G.job(L.cg);
    class_pair((m0 + L.cg) % class_pairs, K, &G.ck, &G.cl);
  }
  G.mu_k = mu_all + mu_at[wjob] + (int64_t)G.ck * G.J.n_t;
  G.mu_l = mu_all + mu_at[wjob] + (int64_t)G.cl * G.J.n_t;
  G.y = y;
  mfma_group_tile<kG>(L, G, x, m_all + (size_t)set * (size_t)p, n, p);
}

// blockIdx.x = macro-tile pair, blockIdx.y = job x class pairs + class pair
__global__ __launch_bounds__(kLanes) void mnewton_cv_mfma_reduce_kernel(const CvCmd* __restrict__ cmd, const CvJob* __restrict__ jobs,
                                                                         const double* __restrict__ part, int class_pairs, int max_chunks,
                                                                         int ncols, double* __restrict__ M_all) {
  const int job = (int)blockIdx.y / class_pairs;
  if (cmd[job].action != kCvStep) return;
  const size_t tile = (size_t)(kT * kT);
  mfma_reduce(part + ((size_t)blockIdx.y * (size_t)max_chunks * gridDim.x + blockIdx.x) * tile, (size_t)gridDim.x * tile, jobs[job].chunks,
              ncols, M_all + (size_t)blockIdx.y * (size_t)ncols * (size_t)ncols);
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
