// The moments pass of the wide Newton cross-validation on the f64 matrix cores (the option "cv_wnewton_moments" = 1;
// newton.hip has the pass it replaces, newton_cv_dense_tile_kernel + newton_cv_reduce_kernel, and says what the moments are).
//
// Job (mix a, training set t) = a * n_sets + t.  For every job whose command of the round is kCvStep: M_job(a, b) =
// sum_i A(i, a) B_job(i, b) over the rows i of the training set, with A = [x - mu_t | 1 | 0] and B_job = [v_job (x - mu_t) |
// v_job | r_job].  The n_mix jobs of one training set read the SAME rows with the SAME centres and differ only in v and r, so
// this is the grouped tile of wide_mfma_device.hpp, which has the geometry.  This unit's own:
//   rows         local row li of the set is row cv_row(J, li): a slab or a chunk may straddle the gap between the set's two
//                row ranges (each lane maps its own row).  The chunks are a function of (n_t, p) alone:
//                wide_mfma_rows_per_chunk(n_t, p + 2), what a single fit with "wnewton_moments" = 1 takes for n_t rows --
//                never of n_mix or of which members step, so a job's bits do not depend on the other jobs of the call or of
//                its group.  A chunk beyond the set's chunks returns at once.
//   weights      loaded from the member's job's v_all / r_all
//   members      kG = kWnewtonCvMfmaGroup consecutive mixes of ONE training set (blockIdx.z = set x groups + group).  The
//                workgroup reads the commands of its group's jobs first: a member takes part only if its action is kCvStep;
//                the M of one that does not step, or is absent (the last group of an n_mix), stays as it is.  A group with
//                no stepping member returns at once.
//   tiles        part[job][chunk][macro pair]; the reduce kernel adds a stepping job's chunks into M[job], entry for entry
//                what newton_cv_reduce_kernel writes
#include "newton_cv_mfma.hpp"

#include "newton.hpp"
#include "wide_mfma_device.hpp"

namespace sgdnet {
namespace {

constexpr int kG = kWnewtonCvMfmaGroup;

struct SetMixes {
  const CvJob J;                         // (the rows and the chunks of a job are its set's: those of mix 0)
  unsigned stepping;                     // bit g: member g (the job (mix0 + g, set)) takes a step in this round
  int mix0, set, n_sets, max_chunks;
  double* part;
  bool weigh = false;
  const double *v = nullptr, *r = nullptr;
  double vi = 0.0, ri = 0.0;
  __device__ bool member(int g) const { return (stepping >> g & 1u) != 0; }
  __device__ size_t job(int g) const { return (size_t)(mix0 + g) * (size_t)n_sets + (size_t)set; }
  __device__ int64_t row(int64_t li, bool live) const { return live ? cv_row(J, li) : 0; }
  __device__ void load(int64_t, int64_t i, bool live) {
    vi = weigh && live ? v[i] : 0.0;
    ri = weigh && live ? r[i] : 0.0;
  }
  __device__ void weights(bool, double& w, double& res) const { w = vi, res = ri; }
  __device__ double* tile(int g) const {
    return part + ((job(g) * (size_t)max_chunks + blockIdx.y) * gridDim.x + blockIdx.x) * (size_t)(kT * kT);
  }
};

__global__ __launch_bounds__(kLanes) void newton_cv_mfma_tile_kernel(const CvCmd* __restrict__ cmd, const CvJob* __restrict__ jobs,
                                                                      const double* __restrict__ x, const double* __restrict__ v_all,
                                                                      const double* __restrict__ r_all, const double* __restrict__ mu_all,
                                                                      int64_t n, int p, int n_sets, int n_mix, int max_chunks,
                                                                      double* __restrict__ part) {
  const int groups = (n_mix + kG - 1) / kG;
  const int set = (int)blockIdx.z / groups, mix0 = ((int)blockIdx.z % groups) * kG;     // the group's first mix
  unsigned stepping = 0;
  for (int g = 0; g < kG; ++g)
    if (mix0 + g < n_mix && cmd[(size_t)(mix0 + g) * (size_t)n_sets + (size_t)set].action == kCvStep) stepping |= 1u << g;
  if (stepping == 0) return;
  SetMixes G{jobs[set], stepping, mix0, set, n_sets, max_chunks, part};
  if ((int)blockIdx.y >= G.J.chunks) return;
  const MfmaTile L(p + 2, G.J.rows_per_chunk, G.J.n_t);
  G.weigh = L.cg < kG && G.member(L.cg);
  const size_t wjob = G.weigh ? G.job(L.cg) : 0;
  G.v = v_all + wjob * (size_t)n;
  G.r = r_all + wjob * (size_t)n;
  mfma_group_tile<kG>(L, G, x, mu_all + (size_t)set * (size_t)p, n, p);
}

// blockIdx.x = macro-tile pair, blockIdx.y = job
__global__ __launch_bounds__(kLanes) void newton_cv_mfma_reduce_kernel(const CvCmd* __restrict__ cmd, const CvJob* __restrict__ jobs,
                                                                        const double* __restrict__ part, int max_chunks, int ncols,
                                                                        double* __restrict__ M_all) {
  const int job = blockIdx.y;
  if (cmd[job].action != kCvStep) return;
  const size_t tile = (size_t)(kT * kT);
  mfma_reduce(part + ((size_t)job * (size_t)max_chunks * gridDim.x + blockIdx.x) * tile, (size_t)gridDim.x * tile, jobs[job].chunks, ncols,
              M_all + (size_t)job * (size_t)ncols * (size_t)ncols);
}

}  // namespace

void wnewton_cv_mfma_moments(const CvCmd* cmd, const CvJob* jobs, const double* x, const double* v_all, const double* r_all,
                             const double* mu_all, int64_t n, int p, int n_sets, int n_mix, int max_chunks, double* part, double* M_all,
                             hipStream_t st) {
  const int ncols = p + 2;
  const unsigned pairs = (unsigned)wide_mfma_pairs(ncols), groups = (unsigned)wnewton_cv_mfma_groups(n_mix);
  hipLaunchKernelGGL(newton_cv_mfma_tile_kernel, dim3(pairs, (unsigned)max_chunks, (unsigned)n_sets * groups), dim3(kLanes), 0, st, cmd, jobs,
                     x, v_all, r_all, mu_all, n, p, n_sets, n_mix, max_chunks, part);
  hipLaunchKernelGGL(newton_cv_mfma_reduce_kernel, dim3(pairs, (unsigned)n_sets * (unsigned)n_mix), dim3(kLanes), 0, st, cmd, jobs, part,
                     max_chunks, ncols, M_all);
}

}  // namespace sgdnet
