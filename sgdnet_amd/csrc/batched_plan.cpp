// Batched SAGA, the host side: which kernel family runs a batch and with what geometry (plan_batch, the one rule), the
// eligibility predicates the solver asks, and the sizes of the fused epoch's buffers.  No kernel lives here.
#include <mutex>
#include <set>
#include <utility>

#include "batched_geometry.hpp"
#include "r_rng_bodies.hpp"

namespace sgdnet {

int batched_max_classes() { return 64; }   // 17..64: sparse x only (binned form, a wavefront per draw)

// The LDS-privatised gather forms pin one workgroup per CU (their tables fill the LDS).  When the
// sample order is generated beside the epoch (solver_rng_*), its G workgroups need CUs of their own:
// a gather launch of 256 workgroups would otherwise wait for them and run a second round (C4: 930
// epochs/s with 256 + 32, 1055 with 224 + 32).  SGDNET_LDS_GRID overrides (experiments).
int lds_target_grid(const SagaDev& d) {
  static const int forced = exp_env_int("SGDNET_LDS_GRID", 0);
  if (forced > 0) return forced;
  const int cus = d.cu_budget > 0 && d.cu_budget < 256 ? d.cu_budget : 256;
  const int g = cus - d.cu_reserve;
  return g < 64 ? 64 : g;
}

size_t binned_max_range_features(int K) { return kRangeLdsBytes / (sizeof(double) * (size_t)K); }

static size_t table_bytes(const SagaDev& d) { return sizeof(double) * (size_t)d.K * (size_t)d.p; }

// Function attributes are per device (one process may drive several GPUs: cv_sgdnet fan-out): the limit is raised
// once per device and kernel, a launch after that makes no HIP call for it but hipGetDevice.
int allow_dynamic_lds(const void* kernel, int bytes) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  static std::mutex mu;
  static std::set<std::pair<const void*, int>> done;
  std::lock_guard<std::mutex> lock(mu);
  if (done.count({kernel, dev})) return SGDNET_OK;
  SGD_HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  done.insert({kernel, dev});
  return SGDNET_OK;
}

// The class width of the kernel instances for K classes: 1, 4, 16 or 64 (17..64 classes: binned and class-lane forms).
static int class_width(int K) { return K == 1 ? 1 : K <= 4 ? 4 : K <= 16 ? 16 : 64; }

// the 8-lane K == 1 form reads two entries per lane: records must hold 16 entries
static bool lanes8_ok(const SagaDev& d) {
  static const int allow = exp_env_int("SGDNET_LANES8", 1);
  return allow && (d.cP || d.rec_cap >= kInReg8) && !SGD_ABLATE(d, ~0);
}

// Compact planes for a K == 1 sparse problem (d.ptr / d.idx / d.val / d.y resident).
bool compact_eligible(const SagaDev& d) {
  static const int allow = exp_env_int("SGDNET_COMPACT", 1);
  if (!allow || d.K != 1 || d.Ky != 1 || d.xd || !d.ptr || d.p > 65536) return false;
  if (2 * sizeof(double) * (size_t)d.p + 16 + kLdsStaticReserve > (size_t)kLdsPerCu) return false;  // no LDS form
  return (double)d.n * 2.0 * kCStride <= 48e9 && d.n < (int64_t)kIdMask;
}

// (a binomial response in another coding -- proportions, -1 / +1: sgdnet_solver_create does not forbid it, only
//  sgdnet_fit_* does -- keeps its value in the record: 11 entries)
int compact_entries(const SagaDev& d) { return d.family == SGDNET_BINOMIAL && d.y_binary ? 12 : 11; }

// Binned form (sparse x): K x p tables that fit no LDS, at batches of 4096 draws and more, and 17..64 classes whatever
// the sizes (the only batched form there).  ensure_binned builds the ranges and sizes the bins when this holds.
bool wants_binned(const SagaDev& d, int64_t batch) {
  static const int allow = exp_env_int("SGDNET_BINNED", 1);
  return allow && !d.xd && d.rec && d.idx && d.K <= 64 && !d.force_global && d.p < (1ll << 31) &&
         (d.K > 16 || (table_bytes(d) > kLdsTableMax && batch >= 4096));
}

// Dense x whose gather hands the batch's gradient changes to an accumulate pass (d.gcb, sized by ensure_dense_tiled):
// K x p tables beyond the LDS, and 17..64 classes whatever the table (the class-lane gather).
bool wants_tiles(const SagaDev& d) { return d.xd && d.K <= 64 && (d.K > 16 || table_bytes(d) > kLdsTableMax); }

// Virtual shards need an LDS gather form: K == 1 with w staged in LDS (sparse or dense x), or 2..16 classes of sparse x
// whose K x p accumulator fits (round 3; the replica of w is read through L2), or dense x (1..16 classes) whose
// accumulator fits.
bool vs_eligible(const SagaDev& d) {
  if (d.V < 2 || d.K < 1 || d.K > 16 || (d.standardize && !(d.vcw && d.c)) || d.force_global || !d.vw) return false;
  const size_t table = table_bytes(d);
  if (d.xd) return table <= kLdsTableMax;                        // only the accumulator is staged
  if (d.K > 1) return d.rec && table <= kLdsTableMax;
  return 2 * table + 16 + kLdsStaticReserve <= kLdsPerCu;     // accumulator + coefficient snapshot in LDS
}

static int vs_grid(const SagaDev& d) { return d.v_bps * d.V; }

// ---- the fused epoch of the virtual shards (saga_vs_epoch_kernel) ----
static int64_t fused_slice(const SagaDev& d) { return 2 * ((d.p + 2 * (int64_t)d.v_bps - 1) / (2 * (int64_t)d.v_bps)); }
static size_t fused_lds_bytes(const SagaDev& d) {
  const int64_t part = (int64_t)(kLdsBlock / 64) * fused_slice(d);     // the slice sweep's per-wavefront partial sums
  return sizeof(double) * (size_t)(d.p + (part > d.p ? part : d.p)) + 16;
}
size_t vs_fused_sync_words() { return (size_t)(kSyncLines + 2) * kSyncLine; }
size_t vs_fused_sync_sticky_word() { return (size_t)kSyncSticky * kSyncLine; }
size_t vs_fused_col_words() { return (size_t)kFusedMaxBps * kSyncLine; }
// local: V reference copies [g_sum | w | g_sum_b | b] + V x 128 c.w partials; published: 2 parities x V slices
size_t vs_fused_exchange_doubles(const SagaDev& d, int n_shards) {
  return (size_t)n_shards * (size_t)(2 * d.p + 2) + (size_t)n_shards * kFusedMaxBps;
}
size_t vs_fused_publish_doubles(const SagaDev& d, int n_shards) { return (size_t)2 * n_shards * (size_t)(2 * d.p + 2); }

// sparse x, one response, compact records, an even number of features, slices of at most 384 features
bool vs_fused_eligible(const SagaDev& d) {
  if (!vs_eligible(d) || d.K != 1 || d.xd || !d.cP || !lanes8_ok(d) || (d.p & 1) || !d.vsync || !d.vx || !d.vcol || !d.vpub) return false;
  if (d.v_bps < 1 || d.v_bps > kFusedMaxBps || d.V * d.v_bps > 1024) return false;
  if (fused_slice(d) > 2 * 64 * kFusedChunks) return false;
  if ((int64_t)d.V * d.v_bps * d.p * 8 >= (1ll << 31)) return false;
  return fused_lds_bytes(d) + kLdsStaticReserve <= kLdsPerCu;
}

// workgroups added to the launch for the sample-order generators (one per reserved CU)
static int vs_fused_rng_workgroups(const SagaDev& d) { return d.rngdev ? d.cu_reserve : 0; }

// How a batch of m draws is launched: the batched iteration's one rule.  The binned form is chosen for the epoch's full
// batch (in.batch), and its tail batch follows.
BatchPlan plan_batch(const SagaDev& d, int m, const PlanInputs& in) {
  BatchPlan g{};
  g.kw = class_width(d.K);
  const size_t table = table_bytes(d);
  if (d.V > 1 && vs_eligible(d)) {      // virtual shards: one launch covers the same batch of all V shards
    const int rng_wgs = vs_fused_rng_workgroups(d);
    g.slab_doubles = (int64_t)vs_grid(d) * d.K * d.p;
    if (in.fused && vs_fused_eligible(d) && vs_grid(d) + rng_wgs <= in.cus) {
      g.form = BatchForm::kFusedEpoch;
      g.grid = vs_grid(d) + rng_wgs;
      g.lds_bytes = fused_lds_bytes(d);
      if (rng_wgs > 0 && g.lds_bytes < kJumpLds) g.lds_bytes = kJumpLds;
      return g;
    }
    g.form = BatchForm::kShards;
    g.grid = vs_grid(d);
    int dpb = (m + d.v_bps - 1) / d.v_bps;
    g.lds_bytes = table;
    if (d.xd) {
      const int waves = (d.K > 1 ? kDenseBlock : kDenseVsBlock) / 64;
      dpb = (dpb + waves - 1) / waves * waves;
    } else {
      const int per_round = kLdsBlock / kGroup;
      if (dpb < per_round) dpb = per_round;
      if (d.K == 1) {
        g.w_lds = true;
        g.lanes8 = lanes8_ok(d);
        g.lds_bytes = 2 * table + 16;
      }
    }
    g.draws_per_block = dpb;
    return g;
  }
  static const int force = [] {
    const char* e = exp_env_str("SGDNET_GATHER");   // "lds" | "global": experiments only
    return !e ? 0 : (e[0] == 'l' ? 1 : 2);
  }();
  const int target_grid = lds_target_grid(d);
  const bool fits = table <= kLdsTableMax;
  if (d.xd) {   // dense x: wave per draw; LDS table + slabs, or the tiled form for larger tables
    const int waves = kDenseBlock / 64;
    if (wants_tiles(d)) {
      g.form = d.K > 16 ? BatchForm::kDenseClassLane : BatchForm::kDenseTiled;
      int dpb = (m + 8191) / 8192;               // a row is >= 5 KB here: one or a few draws per wavefront
      dpb = (dpb + waves - 1) / waves * waves;
      if (dpb < waves) dpb = waves;
      g.draws_per_block = dpb;
      g.grid = (m + dpb - 1) / dpb;
      if (g.grid < 1) g.grid = 1;
      const int64_t tiles = (d.p + kTileF - 1) / kTileF;
      int64_t chunks = (2048 + tiles - 1) / tiles;   // ~2048 workgroups over the chip
      const int64_t most = (m + 4 * waves - 1) / (4 * waves);
      if (chunks > most) chunks = most;
      if (chunks < 1) chunks = 1;
      if (chunks > 65535) chunks = 65535;
      g.draws_per_chunk = (int)((m + chunks - 1) / chunks);
      g.chunks = (int)((m + g.draws_per_chunk - 1) / g.draws_per_chunk);
      // (kept from before the plan: 17..64 classes whose table fits size a slab the class-lane form does not use, and
      //  sgdnet_solver_gather_form answers 1 for them)
      g.slab_doubles = fits ? (int64_t)g.grid * d.K * d.p : 0;
      return g;
    }
    g.form = BatchForm::kDense;
    int dpb = (m + target_grid - 1) / target_grid;
    dpb = (dpb + waves - 1) / waves * waves;
    if (dpb < waves) dpb = waves;
    g.draws_per_block = dpb;
    g.grid = (m + dpb - 1) / dpb;
    if (g.grid < 1) g.grid = 1;
    g.lds_bytes = table;
    // (only more than 64 classes, which no batched launch accepts, leave a table beyond the LDS here)
    g.slab_doubles = fits ? (int64_t)g.grid * d.K * d.p : 0;
    return g;
  }
  // a tail batch of more than 2^20 draws after full batches of fewer is binned (full batches of more are not)
  if (wants_binned(d, in.batch) && d.R > 0 && !in.bins_disabled && force != 2 && m <= (1 << 20)) {
    g.form = BatchForm::kBinned;
    g.draws_per_block = kBinDraws;
    g.grid = (m + kBinDraws - 1) / kBinDraws;
    if (g.grid < 1) g.grid = 1;
    g.lds_bytes = sizeof(BinEntry) * (size_t)kBinEntCap + sizeof(unsigned) * (3 * (size_t)d.R + 1) +
                  ((sizeof(unsigned short) * ((size_t)d.n_coarse + 1) + 15) & ~size_t(15));
    return g;
  }
  // worthwhile once the batch's non-zeros outnumber the table ~48x: below that the fixed
  // cost of writing and re-reading one table per workgroup exceeds the atomics it saves
  const bool pays = (double)m * (double)d.avg_nnz >= 48.0 * (double)d.K * (double)d.p;
  if (!d.force_global && fits && force != 2 && (force == 1 || pays)) {
    g.form = BatchForm::kLds;
    int dpb = (m + target_grid - 1) / target_grid;
    const int per_round = kLdsBlock / kGroup;
    if (dpb < per_round) dpb = per_round;
    g.draws_per_block = dpb;
    g.grid = (m + dpb - 1) / dpb;
    g.lds_bytes = table;
    static const bool w_lds_on = exp_env_int("SGDNET_W_LDS", 1) != 0;
    g.w_lds = d.K == 1 && w_lds_on && 2 * table + kLdsStaticReserve <= kLdsPerCu;
    if (g.w_lds) g.lds_bytes = 2 * table + 16;   // + alignment slack of the second table
    g.lanes8 = g.w_lds && lanes8_ok(d);
  } else {
    g.form = BatchForm::kGlobal;
    g.draws_per_block = kBlock / kGroup;
    g.grid = (m + g.draws_per_block - 1) / g.draws_per_block;
  }
  if (g.grid < 1) g.grid = 1;
  if (g.form == BatchForm::kLds) g.slab_doubles = (int64_t)g.grid * d.K * d.p;
  return g;
}

}  // namespace sgdnet
