// The fit driver's own rules (driver.cpp and driver_direct.cpp obey them): which mode a fit runs in, its first window, how the job is
// cut over the GPUs, shards and generators, and the stability ladder of the automatic window.
//
// Pure functions of shapes, options and a handful of observed numbers: no HIP call, no environment variable, no
// global option is read here (the options come in as FitOptions).  Nothing in this file touches a solver; the
// driver performs what the plan and the guard return.
#pragma once

#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "covariance.hpp"
#include "mnewton.hpp"
#include "newton.hpp"
#include "sgdnet_hip.h"

namespace sgdnet {

// Shortest staleness window the driver uses.  The exported rule (sgdnet_auto_batch) floors at 64 draws, and
// for dense x with a dominant common factor (or few, strongly scaled features) 2 L_max / L_F is well below
// that: a 64-draw window then oscillates or settles on a wrong point without tripping a guard (a random
// sweep of 30-lambda paths found deviance ratios off by 0.06-0.6).  Below 8 draws a batch is no longer
// worth its launch: mode = auto takes the exact iteration there.
constexpr int64_t kWindowFloor = 8;
constexpr int64_t kMaxBatchesPerEpoch = 16384;
constexpr int64_t kRetryWindowMin = kWindowFloor;     // shortest window the divergence restarts go down to

inline std::string plan_text(const char* fmt, ...) {
  char buf[768];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return buf;
}

// 2 L_max / L_F without the exported rule's floor of 64 (kWindowFloor instead); *raw = the unclamped value
inline int64_t window_rule(double max_sample_sqnorm, double l_f, double* raw) {
  *raw = (max_sample_sqnorm > 0.0 && l_f > 0.0) ? 2.0 * max_sample_sqnorm / l_f : 64.0;
  if (!(*raw < 131072.0)) return 131072;
  return *raw < (double)kWindowFloor ? kWindowFloor : (int64_t)*raw;
}

// ---------------------------------------------------------------------------------------------------------------
// FitFacts -> FitPlan
// ---------------------------------------------------------------------------------------------------------------

struct FitOptions {            // sgdnet_set_option values, read by the driver
  int virtual_shards = -1;     // < 0: the rule, 0: off, V: forced
  int rng_generators = 0;      // <= 0: the rule
  int exact_epoch_blocks = 1;
};

struct FitFacts {
  const sgdnet_control* ctl = nullptr;
  bool sparse = false;
  bool on_device = false;      // x was prepared by the device setup passes (the solver adopts it)
  int64_t n = 0, p = 0;
  int n_devices = 0;
  double norm_max = 0.0;       // largest squared row norm
  double l_f = 0.0;            // largest eigenvalue of X'X/n (or its bound); read only where wants_l_f() holds
  FitOptions opt;
};

// SGDNET_MODE_BATCHED means "batched where it is implemented": more than 64 classes run the exact
// iteration instead (a global options(sgdnet.mode = "batched") in R must not make such fits fail);
// (dense x with 17..64 classes: the class-lane form of round 4; until then sgdnet_fit_dense handed it to the sparse entry point)
// An unknown mode comes back as it is (plan_fit refuses it), and so do SGDNET_MODE_COVARIANCE, SGDNET_MODE_NEWTON,
// SGDNET_MODE_MCOVARIANCE, SGDNET_MODE_MNEWTON, SGDNET_MODE_WCOVARIANCE, SGDNET_MODE_WNEWTON and SGDNET_MODE_WMCOVARIANCE: no other mode
// resolves to them.
inline int resolved_mode(int mode, int n_classes) {
  if (mode == SGDNET_MODE_AUTO) mode = SGDNET_MODE_BATCHED;
  if (mode == SGDNET_MODE_BATCHED && n_classes > 64) mode = SGDNET_MODE_EXACT;
  return mode;
}

// The automatic window needs L_F itself.  The device setup passes sample it while they run and ask the control
// block as it came (an unknown mode included); the host Gram pass runs only for a fit that plan_fit will give a window.
inline bool device_setup_wants_l_f(const sgdnet_control& c) { return c.mode != SGDNET_MODE_EXACT && c.batch <= 0; }
inline bool wants_l_f(const sgdnet_control& c) {
  return resolved_mode(c.mode, c.n_classes) == SGDNET_MODE_BATCHED && c.batch <= 0;
}

enum class DrawKind {
  kEpochBlocks,   // exact mode, built-in generator: blocks of several epochs generated on the device
  kPipeline,      // built-in generator: produced in HBM one epoch ahead of the epoch that consumes them
  kHost           // explicit sample_stream or unif callback: filled on the host, uploaded per epoch
};

struct FitPlan {
  int rc = SGDNET_OK;
  std::string error;               // the refusal's text when rc != SGDNET_OK
  int mode = SGDNET_MODE_EXACT;    // the mode actually run
  int64_t window = 0;              // first window (the user's control.batch where there is one)
  int penalty = SGDNET_ELASTICNET;
  // mode = auto left the batched iteration because of the window rule: what the trace line reports
  bool window_refused = false;
  double raw_window = 0.0;
  int64_t batches_per_epoch = 0;
  // rank q runs on rank_dev[q] and holds the samples [rank_lo[q], rank_lo[q + 1])
  int n_ranks = 1;
  std::vector<int> rank_dev;
  std::vector<int64_t> rank_lo;
  DrawKind draws = DrawKind::kHost;
};

inline DrawKind draw_kind(const FitFacts& f, int mode) {
  const sgdnet_control& c = *f.ctl;
  const bool internal = !c.sample_stream && !c.unif;
  if (!internal) return DrawKind::kHost;
  return (mode == SGDNET_MODE_EXACT && !c.debug && f.opt.exact_epoch_blocks) ? DrawKind::kEpochBlocks : DrawKind::kPipeline;
}

// A direct mode solves the path from a Gram or Hessian matrix on the device: no window, no shards, no draws.
inline bool is_direct_mode(int mode) {
  return mode == SGDNET_MODE_COVARIANCE || mode == SGDNET_MODE_NEWTON || mode == SGDNET_MODE_MCOVARIANCE ||
         mode == SGDNET_MODE_MNEWTON || mode == SGDNET_MODE_WCOVARIANCE || mode == SGDNET_MODE_WNEWTON;
}
// SGDNET_MODE_WMCOVARIANCE and SGDNET_MODE_WMNEWTON are planned and run as direct modes too, and plan_fit and the driver ask
// plans_direct().  They are not added to is_direct_mode(): tests/test_direct_plan_host.py records that function over the mode
// numbers 0 .. 9 as "3 .. 8 and no other", and that record stays as it is.
inline bool plans_direct(int mode) { return is_direct_mode(mode) || mode == SGDNET_MODE_WMCOVARIANCE || mode == SGDNET_MODE_WMNEWTON; }

// What differs between the direct modes' refusals; plan_direct asks in this order
struct DirectRule {
  const char* name;            // as "mode = %s" spells it
  int family;
  const char* family_text;
  const char* responses;       // what the number of responses / classes breaks, or nullptr
  int limit;                   // features
  const char* limit_text;
  size_t dense_copy_bytes;     // the driver expands sparse x to a dense copy that stays within this; 0: sparse x is read as it is
  enum { kFeaturesOnly, kClasses, kSamples } prints;   // what the message reports before the features
};

// (P comes with its penalty set; no symbol of the library: driver.cpp and driver_direct.cpp each inline it)
static inline void plan_direct(FitPlan& P, const FitFacts& f, const DirectRule& r) {
  const sgdnet_control& c = *f.ctl;
  const char* what = nullptr;
  if (c.family != r.family) what = r.family_text;
  else if (r.responses) what = r.responses;
  else if (f.p > r.limit) what = r.limit_text;
  else if (c.n_gpus > 1) what = "one GPU (n_gpus <= 1)";
  else if (c.debug) what = "debug = 0 (there are no epochs to report losses of)";
  else if (r.dense_copy_bytes && f.sparse && (double)f.n * (double)f.p * 8.0 > (double)r.dense_copy_bytes)
    what = "the dense copy of a sparse x (n_samples x n_features x 8 bytes) within 1 GiB";
  if (what) {
    std::string shape = plan_text("family %d", c.family);
    if (r.prints != DirectRule::kFeaturesOnly) shape += plan_text(", n_classes %d", c.n_classes);
    if (r.prints == DirectRule::kSamples) shape += plan_text(", %lld samples", (long long)f.n);
    P.rc = SGDNET_EUNSUPPORTED;
    P.error = plan_text("mode = %s needs %s: %s, %lld features (limit %d), n_gpus %d, debug %d", r.name, what, shape.c_str(),
                        (long long)f.p, r.limit, c.n_gpus, c.debug);
    return;
  }
  P.mode = c.mode;
  P.rank_dev.assign(1, c.device);
  P.rank_lo = {0, f.n};                // no window, no shards, no draws
}

inline FitPlan plan_fit(const FitFacts& f) {
  const sgdnet_control& c = *f.ctl;
  const int family = c.family, K = c.n_classes;
  const int64_t n = f.n;
  FitPlan P;

  // penalty functor: sgdnet.cpp:80-98
  if (c.elasticnet_mix == 0.0) P.penalty = SGDNET_RIDGE;
  else if (family == SGDNET_MGAUSSIAN || (family == SGDNET_MULTINOMIAL && c.type_multinomial == 1))
    P.penalty = SGDNET_GROUPLASSO;

  // ---- the direct modes: only where they were asked for (mode = auto must not move existing results; they draw nothing
  // and stop elsewhere than SAGA does), and only for the problem their kernels hold (covariance.hpp, newton.hpp,
  // mnewton.hpp); no silent fall back, neither to SAGA nor from a wide mode to its narrow one ----
  if (plans_direct(c.mode)) {
    const char* one = K != 1 ? "one response (n_classes = 1)" : nullptr;
    switch (c.mode) {
      case SGDNET_MODE_COVARIANCE:      // S in one workgroup's LDS
        plan_direct(P, f, {"covariance", SGDNET_GAUSSIAN, "family = gaussian", one, kCovMaxFeatures,
                           "no more features than sgdnet_covariance_max_features()", 0, DirectRule::kClasses});
        break;
      case SGDNET_MODE_WCOVARIANCE:     // S in global memory: every p from 1 to its own limit
        plan_direct(P, f, {"wcovariance", SGDNET_GAUSSIAN, "family = gaussian", one, kWcovMaxFeatures,
                           "no more features than sgdnet_wcovariance_max_features()", 0, DirectRule::kClasses});
        break;
      case SGDNET_MODE_NEWTON:          // H in one wavefront's LDS
        plan_direct(P, f, {"newton", SGDNET_BINOMIAL, "family = binomial", one, kNewtonMaxFeatures,
                           "no more features than sgdnet_newton_max_features()", 0, DirectRule::kFeaturesOnly});
        break;
      case SGDNET_MODE_WNEWTON:         // H in global memory; sparse x is expanded to a dense copy by the driver
        plan_direct(P, f, {"wnewton", SGDNET_BINOMIAL, "family = binomial", one, kWnewtonMaxFeatures,
                           "no more features than sgdnet_wnewton_max_features()", kWnewtonDenseCopyBytes, DirectRule::kSamples});
        break;
      case SGDNET_MODE_MCOVARIANCE:     // several responses from one Gram matrix
        plan_direct(P, f, {"mcovariance", SGDNET_MGAUSSIAN, "family = mgaussian", nullptr, mcov_max_features(K),
                           "no more features than sgdnet_mcovariance_max_features(n_classes)", 0, DirectRule::kClasses});
        break;
      case SGDNET_MODE_WMCOVARIANCE:    // ... with S in global memory: every p from 1 to its own limit
        plan_direct(P, f, {"wmcovariance", SGDNET_MGAUSSIAN, "family = mgaussian", nullptr, wmcov_max_features(K),
                           "no more features than sgdnet_wmcovariance_max_features(n_classes)", 0, DirectRule::kClasses});
        break;
      default: {                        // SGDNET_MODE_MNEWTON: the joint Hessian in LDS; sparse x as for wnewton
        const char* classes = (K < 2 || K >= 100) ? "2 to 99 classes"
                              : c.type_multinomial != 0 ? "the ungrouped penalty (type_multinomial = 0)" : nullptr;
        if (c.mode == SGDNET_MODE_WMNEWTON)     // ... with the joint Hessian in global memory: every p from 1 to its own limit
          plan_direct(P, f, {"wmnewton", SGDNET_MULTINOMIAL, "family = multinomial", classes, wmnewton_max_features(K),
                             "no more features than sgdnet_wmnewton_max_features(n_classes)", kWmnewtonDenseCopyBytes, DirectRule::kSamples});
        else
          plan_direct(P, f, {"mnewton", SGDNET_MULTINOMIAL, "family = multinomial", classes, mnewton_max_features(K),
                             "no more features than sgdnet_mnewton_max_features(n_classes)", kMNewtonDenseCopyBytes, DirectRule::kSamples});
      }
    }
    return P;
  }

  P.mode = resolved_mode(c.mode, K);
  P.window = c.batch;
  if (P.mode == SGDNET_MODE_BATCHED) {
    if (P.window <= 0) {
      double l_f = f.l_f;
      // dense x takes the dense intercept step (no 0.01 decay): the constant feature is part of the curvature the
      // stale sum has to respect (its mean square is 1; + 1 bounds the largest eigenvalue of the augmented Gram)
      // (standardised dense features are centred: the constant direction is orthogonal to them and the largest
      //  eigenvalue is max(L_F, 1); otherwise the coupling through the column means is bounded by + 1 after the
      //  step-size normalisation by the largest row)
      if (!f.sparse && c.intercept != 0) l_f = c.standardize ? std::max(l_f, 1.0) : l_f + 1.0;
      P.window = window_rule(f.norm_max, l_f, &P.raw_window);
      // ... and so does an epoch of more than kMaxBatchesPerEpoch batches (a short window on many samples): the
      // captured epoch would be a graph of several 10^4 launches, each a few microseconds of fixed cost
      if (c.mode == SGDNET_MODE_AUTO && (P.raw_window < (double)kWindowFloor || n / P.window > kMaxBatchesPerEpoch)) {
        P.window_refused = true;
        P.batches_per_epoch = n / P.window;
        P.mode = SGDNET_MODE_EXACT;
        P.window = 0;
      }
    }
  } else if (P.mode != SGDNET_MODE_EXACT) {
    P.rc = SGDNET_EINVAL;
    P.error = plan_text("unknown mode %d", P.mode);
    return P;
  }

  // ---- the fit sharded over several GPUs of the node (control.n_gpus, ABI 4) ----
  // Rank q holds the samples [q n / N, (q + 1) n / N) on its own GPU with its own virtual shards; the ranks' epoch
  // kernels average ALL replicas among themselves (sgdnet_solver_link_peers).  Rank 0 leads: every rank holds
  // the same coefficients after an epoch, so the path's decisions are taken from it and applied to all.
  const int NG = c.n_gpus > 1 ? c.n_gpus : 1;
  P.n_ranks = NG;
  P.rank_dev.assign((size_t)NG, c.device);
  P.rank_lo.assign((size_t)NG + 1, 0);
  if (NG > 1) {
    if (NG > 8 || !f.sparse || f.on_device || K != 1 || P.mode != SGDNET_MODE_BATCHED || (f.p & 1) || c.debug ||
        c.sample_stream || c.unif) {
      P.rc = SGDNET_EUNSUPPORTED;
      P.error = plan_text("control.n_gpus = %d: a fit is sharded over GPUs in batched mode (mode = batched / auto with a window the "
                          "rule accepts), for sparse x with one response and an even number of features, with the built-in "
                          "generator and without debug losses (at most 8 GPUs)", NG);
      return P;
    }
    for (int q = 0; q < NG; ++q) {
      P.rank_dev[(size_t)q] = c.devices ? c.devices[q] : c.device + q;
      if (P.rank_dev[(size_t)q] < 0 || P.rank_dev[(size_t)q] >= f.n_devices) {
        P.rc = SGDNET_EINVAL;
        P.error = plan_text("control.n_gpus = %d: device %d out of range (%d devices)", NG, P.rank_dev[(size_t)q], f.n_devices);
        return P;
      }
      P.rank_lo[(size_t)q + 1] = n / NG * (q + 1) + std::min<int64_t>(q + 1, n % NG);     // sgdnet_amd/parallel.py: shard_bounds
    }
  }
  P.rank_lo[(size_t)NG] = n;
  P.draws = draw_kind(f, P.mode);
  return P;
}

// 17..64 classes have one batched form, the binned one, and it needs feature ranges (at most 2048 of them): only the
// solver knows whether it has them (solver_batched_available).  Where it has not, the fit runs the exact iteration.
inline void take_exact_iteration(FitPlan& P, const FitFacts& f) {
  P.mode = SGDNET_MODE_EXACT;
  P.window = 0;
  P.draws = draw_kind(f, P.mode);
}

// ---------------------------------------------------------------------------------------------------------------
// Shards and generators
// ---------------------------------------------------------------------------------------------------------------

struct ShardPlan {
  int shards = 0;                 // virtual shards per rank to ask the solvers for; 0: none
  std::vector<int> cu_budget;     // per rank, several ranks only; 0: the whole GPU
  int64_t merge_period = 0;       // several ranks only: draws between two averages
};

// Virtual shards (include/sgdnet_hip.h): with enough samples per feature the batched fit of
// one response (round 3: or of 2..16 classes of sparse x; round 4: of dense x too) runs as up to 8 locally normalised replicas over sample ranges, averaged on the
// device every n / 32 draws -- same optimum, same epochs to tolerance, 2x the epochs per second
// at the benchmark shapes.  sgdnet_set_option("virtual_shards", 0) switches it off, V forces V.
// The shard kernels read a per-shard layout of the sample order: the built-in generator and
// the unif callback produce it (DrawSource::fill), an explicit sample_stream cannot.
// On one GPU the solver may still answer SGDNET_EUNSUPPORTED: the fit then goes on without shards.
inline ShardPlan plan_shards(const FitPlan& P, const FitFacts& f) {
  const sgdnet_control& c = *f.ctl;
  const int K = c.n_classes, NG = P.n_ranks;
  const int64_t n = f.n, p = f.p;
  ShardPlan S;
  // an explicit stream names samples of the whole data set: it cannot be laid out per shard
  if (!(P.mode == SGDNET_MODE_BATCHED && K <= 16 && !c.sample_stream)) return S;
  int V = 1;
  // at least 100 samples per feature in every shard, and a problem large enough for the
  // per-launch cost to matter (small correlated data, e.g. abalone 4177 x 9, converges slower
  // or not at all when its replicas are averaged)
  if (n >= 200000)
    while (V < 8 && (int64_t)(2 * V) * 100 * p <= n) V *= 2;
  // dense x with several classes (round 4): two replicas.  Its windows are a few hundred draws, an epoch is launch-bound
  // and V shards make it V times shorter, but on such well-conditioned data the averaged replicas need more epochs
  // (125 / 213 / 417 at V = 1 / 2 / 4 on 1M x 100, K = 4; profiles/r04_dense_multiclass_vshards.txt): 2 is what pays
  if (!f.sparse && K > 1 && V > 2) V = 2;
  if (f.opt.virtual_shards >= 0) V = f.opt.virtual_shards;
  if (NG > 1) {
    // the job stays a V-way average (8 at most: what the averaging tolerates at these sizes), cut over
    // the ranks -- at least two shards per rank (what the epoch kernel carries)
    V = std::max(2, std::min(8, V) / NG);
    std::vector<int> on_dev((size_t)f.n_devices, 0);
    for (int q = 0; q < NG; ++q) ++on_dev[(size_t)P.rank_dev[(size_t)q]];
    S.cu_budget.assign((size_t)NG, 0);
    for (int q = 0; q < NG; ++q)
      if (on_dev[(size_t)P.rank_dev[(size_t)q]] > 1)          // ranks that share a GPU (rehearsals) share its CUs
        S.cu_budget[(size_t)q] = 256 / on_dev[(size_t)P.rank_dev[(size_t)q]];
    // a quarter of a shard's own epoch between two averages, the same draw count on every rank
    S.merge_period = std::max<int64_t>(1, (n / NG / V) / 4);
    S.shards = V;
  } else if (V >= 2 && V <= 8) {
    S.shards = V;
  }
  return S;
}

// The window once the solvers have taken `shards` shards (0 where they refused):
// at most 1/8 beyond the rule's window when that saves the short last round of every shard's epoch
// (include/sgdnet_hip.h: sgdnet_shard_window; the rule keeps a factor 3 to the unstable regime, profiles/NOTES.md)
inline int64_t shard_window(const FitPlan& P, const FitFacts& f, int shards) {
  if (shards > 1 && f.ctl->batch <= 0 && P.window > 0) return sgdnet_shard_window(P.window, (f.n / P.n_ranks) / shards);
  return P.window;
}

// Generators per rank of the sample-order pipeline.
// batched mode with epochs of 200 000 draws or more: 8-32 generators side by side ON THE ONE
// R STREAM (one makes 10M draws in 5.3 ms, six epochs of the batched kernels at C4): generator g
// starts g * ceil(n / G) draws into the epoch and all of them jump n draws per epoch
// (mt_jump.cpp), so the sample order is set.seed()'s whatever G is.  Smaller problems and exact
// mode keep a single generator.  sgdnet_set_option("rng_generators", G) overrides.
inline int generators_per_rank(const FitPlan& P, const FitFacts& f) {
  int gens = 1;
  if (P.mode == SGDNET_MODE_BATCHED) {
    const int forced = f.opt.rng_generators;
    // a generator's workgroup cannot share a CU with a gather workgroup (LDS and registers are
    // taken), so a long-running generator costs every overlapping gather launch a second round:
    // C4 epochs 1.07 / 0.93 / 0.86 ms with 8 / 16 / 32 generators (0.85 with the stream resident)
    gens = forced > 0 ? forced : (f.n >= 200000 ? (int)std::min<int64_t>(32, std::max<int64_t>(8, f.n / 300000)) : 1);
  }
  return P.n_ranks == 1 ? gens : std::max(2, gens / P.n_ranks);
}

// epochs per block of DrawKind::kEpochBlocks: ~1M draws at a time, 64 epochs at most
inline int64_t block_epochs(int64_t n) { return std::max<int64_t>(1, std::min<int64_t>(64, (1 << 20) / std::max<int64_t>(1, n))); }

// ---------------------------------------------------------------------------------------------------------------
// WindowGuard: the stability ladder of the batched iteration
// ---------------------------------------------------------------------------------------------------------------

struct GuardAction {
  enum What { kGoOn, kAgain, kFail } what = kGoOn;
  // kAgain: this lambda again from the null model
  bool drop_shards = false;     // switch the virtual shards off first
  bool new_budget = false;      // the lambda gets its full max_iter again
  // kFail
  int code = SGDNET_OK;
  std::string message;          // empty: the error text is already set
  bool gave_up = false;         // batched mode gave up: mode = auto reruns the whole fit with the exact iteration
  std::string note;             // SGDNET_TRACE line of the decision, if any
};

class WindowGuard {
 public:
  WindowGuard(const sgdnet_control& c, const FitPlan& P, int64_t window, int shards, double null_dev)
      : batched_(P.mode == SGDNET_MODE_BATCHED), user_batch_(c.batch), n_ranks_(P.n_ranks),
        auto_path_(c.n_lambda_user == 0), null_dev_(null_dev), batch_(window), auto_window_(window), shards_(shards) {}

  int64_t window() const { return batch_; }
  int shards() const { return shards_; }

  // a new lambda starts (or the same one again after the deviance restart): a new step size
  void lambda_starts() {
    if (batched_ && user_batch_ <= 0) batch_ = auto_window_;
    best_ratio_ = HUGE_VAL;
    worse_ = 0;
  }

  // (batched mode) an epoch of lambda li ended, `epochs` of it have run; ch = max|w - w_prev|, sz = max|w|,
  // finite = neither they nor the intercept are NaN or infinite.
  // Guard of the automatic window: the stale-sum step is only stable below ~L_max/L_F
  // draws, and the bound used by sgdnet_auto_batch is optimistic for correlated
  // features.  A change ratio that keeps growing (or stops being finite) halves it.
  GuardAction epoch_ended(int li, unsigned epochs, double ch, double sz, bool finite) {
    GuardAction a;
    const double ratio = change_ratio(ch, sz);
    if (!finite && n_ranks_ > 1) {   // several GPUs: non-finite coefficients are an error at once
      return fail(SGDNET_EUNSUPPORTED, false,
                  plan_text("control.n_gpus = %d: the batched iteration diverged (non-finite coefficients); fit on one GPU, or pass a "
                            "smaller control.batch", n_ranks_));
    }
    if (!finite) {
      // restart this lambda from the null model: first without virtual shards (their
      // averaging assumes shards that look alike), then with a quarter of the window
      if (user_batch_ > 0 && shards_ <= 1)
        return fail(SGDNET_EUNSUPPORTED, false, "batched mode diverged (non-finite coefficients); pass a smaller control.batch");
      if (shards_ > 1) {
        shards_ = 0;
        a.drop_shards = true;
      } else if (batch_ > kRetryWindowMin) {
        // the rule's own floor is 64 draws; a fit that blows up there (few, strongly scaled dense
        // features) gets a shorter window before batched mode is given up
        batch_ = std::max<int64_t>(kRetryWindowMin, batch_ / 4);
        auto_window_ = batch_;
        a.note = plan_text("lambda %d: non-finite coefficients -> window %lld, again", li, (long long)batch_);
      } else {
        return fail(SGDNET_EUNSUPPORTED, true, "batched mode diverged (non-finite coefficients) at the smallest window; use mode = exact");
      }
      a.what = GuardAction::kAgain;   // the epochs run so far stay counted: the lambda does not get its max_iter back
      worse_ = 0;
      best_ratio_ = HUGE_VAL;
      return a;
    }
    // a run on its way out changes the coefficients by a growing, LARGE fraction of their size
    // per epoch; near convergence the ratio is noise around the tolerance and means nothing
    // (without the second condition a 100-lambda path halved its way down to 64 draws)
    // ... and at lambda_max, where the solution is exactly 0, max|w| is rounding noise and the
    // ratio means nothing either (a C3 path spent 54 epochs there halving down to 78 draws)
    const bool at_lambda_max = li == 0 && auto_path_;   // solution exactly 0: no signal (first lambda of an automatic path only)
    if (ratio > 4.0 * best_ratio_ && ratio > 0.05 && sz > 1e-9 && epochs > 2 && !at_lambda_max) ++worse_;
    else worse_ = 0;
    if (ratio > 0.0) best_ratio_ = std::min(best_ratio_, ratio);
    if (worse_ >= 2 && user_batch_ <= 0 && batch_ > kWindowFloor) {
      a.note = plan_text("lambda %d epoch %u: change ratio %.3g after best %.3g -> window %lld halved", li, epochs, ratio,
                         best_ratio_, (long long)batch_);
      batch_ = std::max<int64_t>(kWindowFloor, batch_ / 2);
      // what made the window too long (correlated features) does not depend on lambda: keep
      // it -- except at lambda_max, where a handful of coefficients flicker around zero
      if (li > 0) auto_window_ = batch_;
      worse_ = 0;
      best_ratio_ = ratio;
    }
    return a;
  }

  // binned form: a feature range got more entries in one batch than its bin holds, the epoch is void.
  // More room (or, in the end, the atomic form: grow_rc is what the solver answered when asked for it) and this
  // lambda again from the null model; with more than 16 classes and no room left there is no batched form:
  // mode = auto then fits in exact mode.
  GuardAction bin_overflowed(int li, int grow_rc) {
    if (grow_rc) return fail(grow_rc, true, "");
    GuardAction a;
    a.note = plan_text("lambda %d: a bin overflowed -> more room, again", li);
    // (a cold restart: the warm start of the previous lambda goes too, since the void epoch has been applied to
    //  it; the lambda gets its full max_iter again -- the draws of the void epochs stay consumed, as R's generator
    //  would have it, and are counted in draws_used)
    a.what = GuardAction::kAgain;
    a.new_budget = true;
    worse_ = 0;
    best_ratio_ = HUGE_VAL;
    return a;
  }

  // lambda li ended with this deviance; decreasing = it is smaller than the lambda before it.
  // Safety net of the automatic window: along a decreasing lambda path the deviance of the
  // training data can only fall.  A window that is too long for the data does not have to blow
  // up -- it can settle into a bounded oscillation that the change-ratio guard never sees and
  // that returns a useless fit (deviance above the null model's).  Then: a quarter of the window
  // for the rest of the path, and this lambda again from the null model.
  // ... and whatever the order of a user-supplied lambda sequence: a fit whose deviance is above the
  // null model's (w = 0, intercept only -- the point every lambda can reach) is not a fit.
  GuardAction lambda_ended(int li, double dev, bool decreasing) {
    const bool worse_than_previous = li > 0 && decreasing && dev > prev_dev_ * (1.0 + 1e-3);
    // (a null deviance of exactly 0 -- a constant response -- leaves nothing to compare with: every dev > 0 would
    //  burn the whole ladder)
    const bool worse_than_null = (null_dev_ > 0.0 && dev > null_dev_ * (1.0 + 1e-3)) || !std::isfinite(dev);
    GuardAction a;
    if (batched_ && user_batch_ <= 0 && (worse_than_previous || worse_than_null)) {
      if (batch_ <= kWindowFloor || retries_ >= 8) {
        // the ladder is exhausted and the fit is still worse than a point every lambda can reach: not a fit.
        // mode = auto reruns the whole fit with the exact iteration (sgdnet_fit_*), explicit batched reports it
        return fail(SGDNET_EUNSUPPORTED, true,
                    plan_text("batched mode: the fit at lambda[%d] is worse than %s (deviance %.6g) after %d restarts down to a window of "
                              "%lld draws; use mode = exact", li, worse_than_null ? "the null model" : "the previous lambda's", dev,
                              retries_, (long long)batch_));
      }
      a.note = plan_text("lambda %d: deviance %.6g (previous lambda %.6g, null model %.6g) -> window %lld / 4, again", li, dev,
                         prev_dev_, null_dev_, (long long)batch_);
      if (shards_ > 1 && n_ranks_ == 1) {   // several GPUs keep their shards
        shards_ = 0;
        a.drop_shards = true;
      }
      auto_window_ = std::max<int64_t>(kWindowFloor, batch_ / 4);   // always kept for the rest of the path
      ++retries_;
      a.what = GuardAction::kAgain;   // the lambda is entered again: everything of it starts over
      return a;
    }
    retries_ = 0;
    prev_dev_ = dev;
    return a;
  }

  static double change_ratio(double ch, double sz) { return sz > 0.0 ? ch / sz : 0.0; }

  // for the checks that compare the guard with the rule it replaced
  int64_t auto_window() const { return auto_window_; }
  double best_ratio() const { return best_ratio_; }
  int worse() const { return worse_; }
  int retries() const { return retries_; }
  double prev_dev() const { return prev_dev_; }

 private:
  static GuardAction fail(int code, bool gave_up, std::string message) {
    GuardAction a;
    a.what = GuardAction::kFail;
    a.code = code;
    a.gave_up = gave_up;
    a.message = std::move(message);
    return a;
  }

  const bool batched_;
  const int64_t user_batch_;
  const int n_ranks_;
  const bool auto_path_;
  const double null_dev_;
  int64_t batch_;
  int64_t auto_window_;           // shrinks for good when a run blew up or a fit got worse
  int shards_;
  double best_ratio_ = HUGE_VAL;
  int worse_ = 0;
  int retries_ = 0;
  double prev_dev_ = HUGE_VAL;
};

}  // namespace sgdnet
