// Everything of the solver (solver_state.hpp) that enqueues an epoch on its stream.
//
// The host mirror of LamParams and its upload, the plan of a batch's launches, the launches of a batched epoch
// (separate, sharded or fused; eager or captured), the graph cache, recovery from a fused launch that gave up, and
// the ConvergenceCheck / loss / bin-overflow reads.  Batched epochs are captured once per (batch, draws) shape into a
// hipGraph and replayed, because an epoch is hundreds of microsecond-scale launches (DESIGN.md "Launch structure").
// The entry points that run epochs live here too: sgdnet_solver_run (exact and batched), _enqueue_epochs, _sync,
// _profile_epoch -- all three batched ones start in begin_batched_epochs -- and the synchronous sharded scheme
// (sgdnet_solver_sync_bind / begin / gather / sweep / end).
#include <math.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "solver_state.hpp"

namespace sgdnet {

// what the device copy of `lam` holds, as far as the host can know it (the kernels advance stream_base and
// batch_seq themselves: lam_advance mirrors that; the ConvergenceCheck / loss scratch fields are the device's own)
static bool lam_on_device(const sgdnet_solver* s) {
  if (!s->lam_dev_valid) return false;
  const LamParams &a = s->lam, &b = s->lam_dev_mirror;
  return a.penalty == b.penalty && a.gamma == b.gamma && a.alpha == b.alpha && a.beta == b.beta && a.r_full == b.r_full &&
         a.ls_full == b.ls_full && a.r_tail == b.r_tail && a.ls_tail == b.ls_tail && a.m_full == b.m_full &&
         a.m_tail == b.m_tail && a.stream_base == b.stream_base && a.stream_wrap == b.stream_wrap &&
         a.draws_per_epoch == b.draws_per_epoch && a.batch_seq == b.batch_seq && a.stream_raw == b.stream_raw &&
         a.rng_generate == b.rng_generate;
}

// host mirror of end_epoch (batched_device.hpp)
static void lam_advance(sgdnet_solver* s, int64_t draws, int batches) {
  for (LamParams* q : {&s->lam, &s->lam_dev_mirror}) {
    int64_t sb = q->stream_base + draws;
    if (q->stream_wrap > 0 && sb >= q->stream_wrap) sb -= q->stream_wrap;
    q->stream_base = sb;
    q->batch_seq += batches;
  }
}

// Uploads `lam` unless the device already holds exactly these values: back-to-back epochs of one lambda then
// run graph after graph with no copy in between (the 120-byte upload is a blit kernel of ~20 us on the solver's
// stream: 2 % of a C4 epoch).
int push_lam(sgdnet_solver* s) {
  if (lam_on_device(s)) return SGDNET_OK;
  const int slot = s->lam_slot;
  s->lam_slot = (slot + 1) % sgdnet_solver::kLamSlots;
  SGD_HIP_TRY(hipEventSynchronize(s->lam_ev[slot]));   // the slot's previous upload has completed
  s->lam_stage[slot] = s->lam;
  SGD_HIP_TRY(hipMemcpyAsync(s->lam_dev, &s->lam_stage[slot], sizeof(LamParams), hipMemcpyHostToDevice,
                             s->st));
  SGD_HIP_TRY(hipEventRecord(s->lam_ev[slot], s->st));
  s->lam_dev_mirror = s->lam;
  s->lam_dev_valid = true;
  return SGDNET_OK;
}

// r^m and LS_m = sum_{k<m} r^k for r = 1 - alpha*gamma: closed form of the
// reference's cumulative lag_scaling table (src/saga-sparse.h:229-240).
static void batch_factors(double alpha, double gamma, int64_t m, double* r_m, double* ls_m) {
  const double a = 1.0 - (1.0 - alpha * gamma);  // 1 - r, exact for the rounded r
  if (a == 0.0) {
    *r_m = 1.0;
    *ls_m = (double)m;
  } else {
    const double e = expm1((double)m * log1p(-a));  // r^m - 1
    *r_m = 1.0 + e;
    *ls_m = -e / a;
  }
}

void drop_graph(sgdnet_solver* s) {
  for (auto& g : s->graphs) {
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
    if (g.graph) (void)hipGraphDestroy(g.graph);
  }
  s->graphs.clear();
  s->gexec = nullptr;
}

// The launches of an epoch in batches of `batch` draws: m = batch for a full batch, the tail's draws for the tail batch.
BatchPlan plan(const sgdnet_solver* s, int64_t batch, int64_t m) {
  return plan_batch(s->d, (int)m, PlanInputs{batch, s->bin_disabled, !s->fused_off && option(kOptFusedEpoch) != 0, s->cus});
}
static bool sharded(const BatchPlan& g) { return g.form == BatchForm::kShards || g.form == BatchForm::kFusedEpoch; }
// (whether the epoch is one fused launch does not depend on the batch)
bool fused_epochs(const sgdnet_solver* s) { return plan(s, 1, 1).form == BatchForm::kFusedEpoch; }

static int set_batch_shape(sgdnet_solver* s, int64_t batch, int64_t draws) {
  if (batch < 1) batch = 1;
  {
    const int rcm = m_to_record(s);          // batched kernels: the gradient memory rides in the records
    if (rcm) return rcm;
  }
  const bool shards = sharded(plan(s, batch, batch));
  const int64_t per_launch = shards ? draws / s->d.V : draws;   // virtual shards: per-shard batches, V in a launch
  if (shards) s->d.v_dps = per_launch;
  if (batch > per_launch) batch = per_launch;
  if (!shards) {
    int rcb = ensure_binned(s, batch);
    if (!rcb) rcb = ensure_dense_tiled(s, batch);
    if (rcb) return rcb;
  }
  // scratch must cover the full batches AND the tail batch, whose launch geometry (and even
  // its gather form) can differ
  const int64_t full = per_launch / batch;
  const int64_t tail = per_launch - full * batch;
  int64_t slab_need = plan(s, batch, batch).slab_doubles;
  if (tail > 0) slab_need = std::max(slab_need, plan(s, batch, tail).slab_doubles);
  if (slab_need > s->slab_cap) {
    SGD_HIP_TRY(hipStreamSynchronize(s->st));
    if (s->d.slab) SGD_HIP_TRY(hipFree(s->d.slab));
    s->d.slab = nullptr;
    SGD_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&s->d.slab), sizeof(double) * (size_t)slab_need));
    s->slab_cap = slab_need;
    drop_graph(s);
  }
  s->lam.m_full = batch;
  s->lam.m_tail = tail;
  batch_factors(s->lam.alpha, s->lam.gamma, batch, &s->lam.r_full, &s->lam.ls_full);
  batch_factors(s->lam.alpha, s->lam.gamma, tail, &s->lam.r_tail, &s->lam.ls_tail);
  s->lam.draws_per_epoch = draws;
  return SGDNET_OK;
}

static int n_batches(int64_t batch, int64_t draws) {
  if (batch < 1) batch = 1;
  if (batch > draws) batch = draws;
  return (int)((draws + batch - 1) / batch);
}

// ---- virtual shards (DESIGN.md 8 "one GPU") ----------------------------------------------------
// `draws` is the epoch's total; every shard does draws / V of them in batches of `batch`, all
// shards' k-th batch in one gather + one sweep launch; the replicas are averaged every
// vs_merge_batches batches and at the end of the epoch.
static int vs_merge_batches(const sgdnet_solver* s, int64_t batch) {
  // draws per shard between merges: n / 32 of the job (parallel.py), settable for sharded jobs
  const int64_t period = s->vs_period > 0 ? s->vs_period : s->d.n / 32;
  const int64_t b = period / batch;
  return (int)(b < 1 ? 1 : b);
}

// Dispatch-level start / stop events of one launch (no host gaps inside the interval) where somebody asked for its
// time, nullptrs where nobody did.  The pair belongs to `owner` before the launch it brackets: a launch that fails
// leaks nothing.  `pool` (optional): events to take before any is created.
static int timing_pair(std::vector<hipEvent_t>* owner, hipEvent_t* e0, hipEvent_t* e1,
                       std::vector<hipEvent_t>* pool = nullptr) {
  *e0 = *e1 = nullptr;
  if (!owner) return SGDNET_OK;
  for (hipEvent_t* e : {e0, e1}) {
    if (pool && !pool->empty()) {
      *e = pool->back();
      pool->pop_back();
    } else {
      SGD_HIP_TRY(hipEventCreate(e));
    }
    owner->push_back(*e);
  }
  return SGDNET_OK;
}

// sgdnet_solver_epoch_timing(enable): the events of the launches to come are made now, not between them
constexpr size_t kTimedLaunchesAhead = 64;
static int fill_event_pool(sgdnet_solver* s) {
  while (s->ev_pool.size() < 2 * kTimedLaunchesAhead) {
    hipEvent_t e = nullptr;
    SGD_HIP_TRY(hipEventCreate(&e));
    s->ev_pool.push_back(e);
  }
  return SGDNET_OK;
}

// The whole epoch in one launch (batched_shards.hip "Fused epoch", BatchForm::kFusedEpoch): option fused_epoch, the
// kernel's own limits, a device with at least as many CUs as the launch has workgroups, and no earlier launch of this
// solver that failed to become resident.
// `ev` (sgdnet_solver_profile_epoch) receives four events per gather + sweep pair; for the fused launch its pair and an
// empty interval.  Without it the fused launch is still timed when sgdnet_solver_epoch_timing asked (epoch_ev).
static int enqueue_epoch_kernels_vs(sgdnet_solver* s, int64_t batch, int64_t draws, std::vector<hipEvent_t>* ev) {
  SagaDev& d = s->d;
  const int64_t dps = draws / d.V;
  if (batch > dps) batch = dps;
  const int nb = n_batches(batch, dps);
  const BatchPlan full = plan(s, batch, batch);
  const int every = vs_merge_batches(s, batch);
  if (full.form == BatchForm::kFusedEpoch) {
    s->d.vs_xcd_local = option(kOptFusedEpoch) == 1 ? 1 : 0;
    hipEvent_t e0, e1;
    int rcf = timing_pair(ev ? ev : s->time_epochs ? &s->epoch_ev : nullptr, &e0, &e1, ev ? nullptr : &s->ev_pool);
    if (!rcf) rcf = launch_vs_epoch(d, full, s->lam_dev, nb, every, s->st, e0, e1);
    if (rcf || !ev) return rcf;
    hipEvent_t z0, z1;                          // no separate sweep launches: an empty interval
    rcf = timing_pair(ev, &z0, &z1);
    if (rcf) return rcf;
    SGD_HIP_TRY(hipEventRecord(z0, s->st));
    SGD_HIP_TRY(hipEventRecord(z1, s->st));
    return SGDNET_OK;
  }
  const BatchPlan tail_plan = plan(s, batch, dps - (int64_t)(nb - 1) * batch);
  int rc = launch_vs_broadcast(d, s->st);
  if (rc) return rc;
  rc = launch_vs_cw(d, s->st);
  if (rc) return rc;
  for (int k = 0; k < nb; ++k) {
    const int64_t t0 = (int64_t)k * batch;
    const int64_t m = (dps - t0 < batch) ? dps - t0 : batch;
    const int tail = (m != batch) ? 1 : 0;
    const BatchPlan& g = tail ? tail_plan : full;
    hipEvent_t g0, g1, w0, w1;
    rc = timing_pair(ev, &g0, &g1);
    if (!rc) rc = timing_pair(ev, &w0, &w1);
    if (rc) return rc;
    rc = launch_vs_gather(d, g, s->lam_dev, t0, (int)m, s->st, g0, g1, k);
    if (rc) return rc;
    rc = launch_vs_sweep(d, g, s->lam_dev, tail, s->st, w0, w1);
    if (rc) return rc;
    const bool last = k + 1 == nb;
    if (last || (k + 1) % every == 0) {
      rc = launch_vs_merge(d, last ? 1 : 0, s->st, last ? s->lam_dev : nullptr, nb);   // the last one also ends the epoch
      if (rc) return rc;
    }
    if (!last) {
      rc = launch_vs_cw(d, s->st);                // c . w of the replicas the next gather reads
      if (rc) return rc;
    }
  }
  return SGDNET_OK;
}

// Enqueue the kernels of one batched epoch (eager or under stream capture).
static int enqueue_epoch_kernels(sgdnet_solver* s, int64_t batch, int64_t draws, std::vector<hipEvent_t>* ev) {
  if (batch < 1) batch = 1;
  if (sharded(plan(s, batch, batch))) return enqueue_epoch_kernels_vs(s, batch, draws, ev);
  if (batch > draws) batch = draws;
  const int nb = n_batches(batch, draws);
  const BatchPlan full = plan(s, batch, batch);
  const BatchPlan tail_plan = plan(s, batch, draws - (int64_t)(nb - 1) * batch);
  // the launch geometry must fit the scratch sized by set_batch_shape (a mismatch would
  // write past d0_part / slab on the device)
  for (const BatchPlan* g : {&full, &tail_plan})
    if (g->slab_doubles > s->slab_cap) {
      set_error("internal: gather geometry of a batch exceeds its scratch");
      return SGDNET_EINVAL;
    }
  // (as before the plan: the coefficient copy is refreshed when the FULL batches are binned -- a binned tail batch
  //  after full batches of more than 2^20 draws finds it as the last binned epoch left it)
  if (full.form == BatchForm::kBinned) {
    const int rcw = launch_wpad_refresh(s->d, s->st);
    if (rcw) return rcw;
  }
  for (int k = 0; k < nb; ++k) {
    const int64_t t0 = (int64_t)k * batch;
    const int64_t m = (draws - t0 < batch) ? draws - t0 : batch;
    const int tail = (m != batch) ? 1 : 0;
    const BatchPlan& g = tail ? tail_plan : full;
    hipEvent_t g0, g1, w0, w1;
    int rc = timing_pair(ev, &g0, &g1);
    if (!rc) rc = timing_pair(ev, &w0, &w1);
    if (rc) return rc;
    rc = launch_batch_gather(s->d, g, s->lam_dev, t0, (int)m, k, s->st, g0, g1);
    if (rc) return rc;
    rc = launch_batch_sweep(s->d, g, s->lam_dev, s->lam.penalty, tail, k, s->st, w0, w1);
    if (rc) return rc;
  }
  return launch_epoch_end(s->lam_dev, nb, s->st);
}

static int ensure_graph(sgdnet_solver* s, int64_t batch, int64_t draws) {
  const int fused = fused_epochs(s) ? option(kOptFusedEpoch) : 0;
  for (auto& g : s->graphs)
    if (g.batch == batch && g.draws == draws && g.fused == fused) {
      s->gexec = g.exec;
      s->fused_in_graph = fused != 0;
      return SGDNET_OK;
    }
  if (s->graphs.size() >= 4) {   // a sharded epoch uses at most two shapes (segments + remainder)
    auto& old = s->graphs.front();
    SGD_HIP_TRY(hipStreamSynchronize(s->st));
    (void)hipGraphExecDestroy(old.exec);
    (void)hipGraphDestroy(old.graph);
    s->graphs.erase(s->graphs.begin());
  }
  s->fused_in_graph = fused != 0;
  SGD_HIP_TRY(hipStreamBeginCapture(s->st, hipStreamCaptureModeThreadLocal));
  // (a captured launch does not run: it gets no timing events -- a pair that is never recorded has no interval, and
  //  the failed hipEventElapsedTime would stay behind as the thread's last error for the next launch to find)
  const bool timed = s->time_epochs;
  s->time_epochs = false;
  int rc = enqueue_epoch_kernels(s, batch, draws, nullptr);
  s->time_epochs = timed;
  hipGraph_t g = nullptr;
  hipError_t e = hipStreamEndCapture(s->st, &g);
  if (rc) {
    if (g) (void)hipGraphDestroy(g);
    return rc;
  }
  if (e != hipSuccess) {
    set_error("hipStreamEndCapture failed: %s", hipGetErrorString(e));
    return SGDNET_EHIP;
  }
  hipGraphExec_t ex = nullptr;
  e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
  if (e != hipSuccess) {
    (void)hipGraphDestroy(g);
    set_error("hipGraphInstantiate failed: %s", hipGetErrorString(e));
    return SGDNET_EHIP;
  }
  s->graphs.push_back({batch, draws, g, ex, fused});
  s->gexec = ex;
  return SGDNET_OK;
}

// One epoch on the solver's stream: the captured graph -- or, where the epoch is ONE kernel anyway (fused epoch of the
// virtual shards), that launch itself: a one-node graph replay left ~14 us between two epochs, a plain launch ~2.
static int launch_epoch(sgdnet_solver* s, int64_t batch, int64_t draws) {
  if (s->fused_in_graph) return enqueue_epoch_kernels(s, batch, draws, nullptr);
  SGD_HIP_TRY(hipGraphLaunch(s->gexec, s->st));
  return SGDNET_OK;
}

static int check_batched_ok(const sgdnet_solver* s) {
  if (s->d.K > batched_max_classes()) {
    set_error("batched mode supports n_classes <= %d (got %d)", batched_max_classes(), s->d.K);
    return SGDNET_EUNSUPPORTED;
  }
  if (!s->sparse) {
    // dense x: one LDS copy of the K x p accumulator per workgroup (saga_batch_gather_dense_kernel), the tiled form when
    // that copy fits no LDS, the class-lane form for 17..64 classes
    return SGDNET_OK;
  }
  if (!s->d.rec) {
    set_error("batched mode: packed sample records were not built");
    return SGDNET_EUNSUPPORTED;
  }
  return SGDNET_OK;
}

static int check_stream(const sgdnet_solver* s, int64_t off, int64_t need) {
  if (!s->stream_dev || off < 0 || off + need > s->stream_len) {
    set_error("sample stream too short: need [%lld, %lld) but %lld entries are resident",
              (long long)off, (long long)(off + need), (long long)s->stream_len);
    return SGDNET_ESTREAM;
  }
  return SGDNET_OK;
}

static int read_convergence(sgdnet_solver* s, double tol, int* converged) {
  LamParams back;
  SGD_HIP_TRY(hipMemcpyAsync(&back, s->lam_dev, sizeof(LamParams), hipMemcpyDeviceToHost, s->st));
  SGD_HIP_TRY(hipStreamSynchronize(s->st));
  double max_change, max_size;
  memcpy(&max_change, &back.max_change_bits, 8);
  memcpy(&max_size, &back.max_size_bits, 8);
  const bool all_zero = (max_size == 0.0) && (max_change == 0.0);
  const bool no_change = (max_size != 0.0) && (max_change / max_size <= tol);
  *converged = (all_zero || no_change) ? 1 : 0;
  s->last_change = max_change;
  s->last_size = max_size;
  s->fused_abort_seen = back.fused_abort;
  return SGDNET_OK;
}

// A fused epoch launch that gave up (batched_shards.hip "Fused epoch").  *rerun: the launch changed nothing, the
// caller runs the epoch again (the solver has switched to separate launches).
static int fused_recover(sgdnet_solver* s, int code, int64_t draws, int batches, bool* rerun) {
  *rerun = false;
  if (!code) return SGDNET_OK;
  s->fused_off = true;
  s->fused_abort_seen = 0;
  SGD_HIP_TRY(hipMemsetAsync(reinterpret_cast<char*>(s->lam_dev) + offsetof(LamParams, fused_abort), 0, sizeof(int), s->st));
  SGD_HIP_TRY(hipMemsetAsync(s->d.vsync + vs_fused_sync_sticky_word(), 0, sizeof(unsigned), s->st));
  if (code != 1) {
    set_error("batched mode: a wait inside the fused epoch kernel timed out (internal error; the epoch is void)");
    return SGDNET_EHIP;
  }
  if (s->d.n_peers > 1) {                       // the separate launches know nothing of the other ranks
    set_error("batched mode: the epoch kernel of a linked solver could not become resident on its GPU (shared with other "
              "work?); the ranks' replicas are averaged inside that kernel, so there is no fallback");
    return SGDNET_EHIP;
  }
  if (getenv("SGDNET_TRACE"))
    fprintf(stderr, "[sgdnet]   the fused epoch launch could not become resident (GPU shared?): separate launches from now on\n");
  // the device did not advance the epoch's bookkeeping: take the host mirror back
  for (LamParams* q : {&s->lam, &s->lam_dev_mirror}) {
    int64_t sb = q->stream_base - draws;
    if (sb < 0 && q->stream_wrap > 0) sb += q->stream_wrap;
    q->stream_base = sb;
    q->batch_seq -= batches;
  }
  if (s->lam.stream_raw) {                      // the slot holds raw words: the separate launches read draws
    int rc = stream_to_draws(s, s->lam.stream_base, s->pipe.n);
    if (rc) return rc;
    s->lam.stream_raw = 0;
  }
  *rerun = true;
  return SGDNET_OK;
}

static int device_convergence(sgdnet_solver* s, double tol, int* converged) {
  const size_t off = offsetof(LamParams, max_change_bits);
  SGD_HIP_TRY(hipMemsetAsync(reinterpret_cast<char*>(s->lam_dev) + off, 0, 16, s->st));
  int rc = launch_convergence(s->d, s->lam_dev, s->st);
  if (rc) return rc;
  return read_convergence(s, tol, converged);
}

int device_loss_sum(sgdnet_solver* s, double* out) {
  const size_t off = offsetof(LamParams, loss_acc);
  SGD_HIP_TRY(hipMemsetAsync(reinterpret_cast<char*>(s->lam_dev) + off, 0, 8, s->st));
  int rc = launch_loss(s->d, s->lam_dev, s->sparse, s->st);
  if (rc) return rc;
  SGD_HIP_TRY(hipMemcpyAsync(out, reinterpret_cast<char*>(s->lam_dev) + off, 8, hipMemcpyDeviceToHost,
                             s->st));
  SGD_HIP_TRY(hipStreamSynchronize(s->st));
  return SGDNET_OK;
}

static int ensure_ls_table(sgdnet_solver* s, int64_t nit) {
  if (s->LS_dev && s->LS_len == nit + 1 && s->LS_alpha == s->lam.alpha && s->LS_gamma == s->lam.gamma)
    return SGDNET_OK;
  // saga-sparse.h:229-240, same sequential arithmetic
  std::vector<double> ls((size_t)(nit + 1 > 2 ? nit + 1 : 2));
  ls[0] = 0.0;
  ls[1] = 1.0;
  double geo = 1.0;
  const double upd = 1.0 - s->lam.alpha * s->lam.gamma;
  for (int64_t i = 2; i < nit + 1; ++i) {
    geo *= upd;
    ls[(size_t)i] = ls[(size_t)i - 1] + geo;
  }
  if (!s->LS_dev || s->LS_len != nit + 1) {
    if (s->LS_dev) {
      SGD_HIP_TRY(hipStreamSynchronize(s->st));
      SGD_HIP_TRY(hipFree(s->LS_dev));
      s->LS_dev = nullptr;
    }
    SGD_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&s->LS_dev), sizeof(double) * ls.size()));
  }
  SGD_HIP_TRY(hipMemcpy(s->LS_dev, ls.data(), sizeof(double) * ls.size(), hipMemcpyHostToDevice));
  s->LS_len = nit + 1;
  s->LS_alpha = s->lam.alpha;
  s->LS_gamma = s->lam.gamma;
  return SGDNET_OK;
}

// binned form: a bin that overflowed dropped entries -- the epoch's result is not the algorithm's
static int check_bins(sgdnet_solver* s) {
  if (s->d.R <= 0 || !s->d.bins || !s->d.bin_err) return SGDNET_OK;
  int flag = 0;
  SGD_HIP_TRY(hipMemcpyAsync(&flag, s->d.bin_err, sizeof(int), hipMemcpyDeviceToHost, s->st));
  SGD_HIP_TRY(hipStreamSynchronize(s->st));
  if (flag) {
    SGD_HIP_TRY(hipMemsetAsync(s->d.bin_err, 0, sizeof(int), s->st));
    s->bin_overflowed = true;       // sgdnet_fit_* recovers (solver_grow_bins); a direct caller sees the error
    set_error("batched mode (binned form): a feature range received more entries in one batch than its bin holds "
              "(the epochs since the last synchronisation are void); pass a smaller batch");
    return SGDNET_EUNSUPPORTED;
  }
  return SGDNET_OK;
}

// What every batched entry point does before its first epoch, in this order on the solver's stream.  The order is
// behaviour: m_to_record (set_batch_shape) drops graphs, prepare_stream_slot decides stream_raw / rng_generate before
// the upload, lam_on_device decides whether there is an upload at all.  `stream_need`: the entries from
// `stream_offset` on that the caller is about to read; `n_epochs`: the epochs it may enqueue before it comes back.
// *batch_out: the batch as the launches take it.
static int begin_batched_epochs(sgdnet_solver* s, int64_t batch, int64_t stream_offset, int64_t stream_need,
                                int64_t draws_per_epoch, int n_epochs, int64_t* batch_out) {
  int rc = check_batched_ok(s);
  if (rc) return rc;
  rc = check_stream(s, stream_offset, stream_need);
  if (rc) return rc;
  if (batch < 1) batch = 1;
  if (batch > draws_per_epoch) batch = draws_per_epoch;
  *batch_out = batch;
  rc = set_batch_shape(s, batch, draws_per_epoch);
  if (rc) return rc;
  s->lam.stream_base = stream_offset;
  s->lam.stream_wrap = stream_wrap_for(s, stream_offset, draws_per_epoch);
  rc = prepare_stream_slot(s, batch, stream_offset, draws_per_epoch, n_epochs);
  if (rc) return rc;
  rc = push_lam(s);
  if (rc) return rc;
  if (s->d.standardize) rc = launch_cw_init(s->d, s->lam_dev, s->st);
  return rc;
}

}  // namespace sgdnet

using namespace sgdnet;

bool solver_fused_aborted(const sgdnet_solver* s) { return s && s->fused_abort_seen != 0; }

extern "C" {

int sgdnet_solver_run(sgdnet_solver* s, int mode, int64_t batch, int64_t stream_offset,
                      int64_t draws_per_epoch, unsigned max_epochs, double tol, unsigned* epochs_run,
                      int* converged_out, double* losses) {
  if (!s || draws_per_epoch <= 0 || max_epochs == 0 || !epochs_run || !converged_out) {
    set_error("sgdnet_solver_run: invalid argument");
    return SGDNET_EINVAL;
  }
  if (!s->penalty_set) {
    set_error("sgdnet_solver_run: call sgdnet_solver_set_penalty first");
    return SGDNET_EINVAL;
  }
  SGD_HIP_TRY(hipSetDevice(s->device));
  int rc = check_stream(s, stream_offset, draws_per_epoch);
  if (rc) return rc;
  const size_t wbytes = sizeof(double) * (size_t)s->d.K * (size_t)s->d.p;
  unsigned done = 0;
  int converged = 0;

  if (mode == SGDNET_MODE_EXACT) {
    rc = m_to_array(s);                       // the exact kernels read the K x n gradient memory
    if (rc) return rc;
    rc = stream_to_draws(s, stream_offset, s->stream_len - stream_offset);
    if (rc) return rc;
    if (s->sparse) {
      rc = ensure_ls_table(s, draws_per_epoch);
      if (rc) return rc;
    }
    ExactPlan plan;
    rc = plan_exact(s->d, ExactInputs{s->sparse, draws_per_epoch, s->lam.penalty, s->lam.alpha, s->lam.gamma, s->nnz,
                                      option(kOptExactRowRegisters)}, &plan);
    if (rc) return rc;
    while (done < max_epochs && !converged) {
      const int64_t avail = (s->stream_len - stream_offset) / draws_per_epoch;
      if (avail <= 0) {
        set_error("sample stream exhausted after %u epochs", done);
        return SGDNET_ESTREAM;
      }
      unsigned chunk = max_epochs - done;
      if ((int64_t)chunk > avail) chunk = (unsigned)avail;
      if (losses) chunk = 1;  // per-epoch loss needs a launch boundary
      ExactCtl ctl{};
      ctl.stream_off = stream_offset;
      ctl.nit = draws_per_epoch;
      ctl.max_epochs = chunk;
      ctl.tol = tol;
      ctl.LS = s->LS_dev;
      ctl.use_lds = plan.use_lds;
      ctl.ls_cache = plan.ls_cache;
      ctl.out = s->out_dev;
      rc = launch_exact(s->d, plan, s->lam_dev, ctl, s->st);
      if (rc) return rc;
      int out[2] = {0, 0};
      SGD_HIP_TRY(hipMemcpyAsync(out, s->out_dev, sizeof(out), hipMemcpyDeviceToHost, s->st));
      SGD_HIP_TRY(hipStreamSynchronize(s->st));
      if (out[1] < 0) {
        set_error("exact mode: the sample-order producer of the sparse kernel stalled (internal error)");
        return SGDNET_EHIP;
      }
      if (losses) {
        double sum = 0.0;
        rc = device_loss_sum(s, &sum);
        if (rc) return rc;
        losses[done] = sum / (double)s->d.n;
      }
#ifdef SGDNET_PHASE_TIMING
      rc = phase_report_exact(s, plan, out[0], draws_per_epoch);
      if (rc) return rc;
#endif
      done += (unsigned)out[0];
      converged = out[1];
      stream_offset += (int64_t)out[0] * draws_per_epoch;
    }
    s->w_prev_valid = true;
  } else if (mode == SGDNET_MODE_BATCHED) {
    // (the stream holds the first epoch, checked above and again per epoch: later epochs may exhaust it)
    rc = begin_batched_epochs(s, batch, stream_offset, draws_per_epoch, draws_per_epoch, (int)max_epochs, &batch);
    if (rc) return rc;
    // ConvergenceCheck{w, tol}: w_prev starts as the warm-start w (saga-sparse.h:251)
    SGD_HIP_TRY(hipMemcpyAsync(s->d.w_prev, s->d.w, wbytes, hipMemcpyDeviceToDevice, s->st));
    rc = ensure_graph(s, batch, draws_per_epoch);
    if (rc) return rc;
    const int nb = n_batches(batch, draws_per_epoch);
    while (done < max_epochs && !converged) {
      rc = check_stream(s, s->lam.stream_base, draws_per_epoch);
      if (rc) return rc;
      const auto tl0 = std::chrono::steady_clock::now();
      const bool tr = getenv("SGDNET_TRACE") != nullptr;
      if (tr && !s->trace_ev[0])                // (the solver's device is current)
        for (hipEvent_t& e : s->trace_ev) (void)hipEventCreate(&e);
      if (tr) (void)hipEventRecord(s->trace_ev[0], s->st);
      rc = launch_epoch(s, batch, draws_per_epoch);
      if (rc) return rc;
      if (tr) (void)hipEventRecord(s->trace_ev[1], s->st);
      s->trace_launch += std::chrono::duration<double>(std::chrono::steady_clock::now() - tl0).count();
      lam_advance(s, draws_per_epoch, nb);     // mirrors end_epoch on the device
      if (losses) {
        double sum = 0.0;
        rc = device_loss_sum(s, &sum);
        if (rc) return rc;
        losses[done] = sum / (double)s->d.n;
      }
      const auto tc0 = std::chrono::steady_clock::now();
      rc = device_convergence(s, tol, &converged);
      if (rc) return rc;
      if (s->fused_in_graph && s->fused_abort_seen) {
        bool rerun = false;
        rc = fused_recover(s, s->fused_abort_seen, draws_per_epoch, nb, &rerun);
        if (rc) return rc;
        if (rerun) {                            // nothing was modified: the same epoch as separate launches
          converged = 0;
          rc = ensure_graph(s, batch, draws_per_epoch);
          if (rc) return rc;
          continue;
        }
      }
      rc = check_bins(s);
      if (rc) return rc;
      s->trace_conv += std::chrono::duration<double>(std::chrono::steady_clock::now() - tc0).count();
      if (tr) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, s->trace_ev[0], s->trace_ev[1]) == hipSuccess) s->trace_graph += ms * 1e-3;
      }
      ++s->trace_epochs;
      ++done;
    }
    s->w_prev_valid = true;
  } else {
    set_error("unknown mode %d", mode);
    return SGDNET_EINVAL;
  }
  *epochs_run = done;
  *converged_out = converged;
  return SGDNET_OK;
}

int sgdnet_solver_enqueue_epochs(sgdnet_solver* s, int64_t batch, int64_t stream_offset,
                                 int64_t draws_per_epoch, int n_epochs) {
  if (!s || draws_per_epoch <= 0 || n_epochs <= 0 || !s->penalty_set) {
    set_error("sgdnet_solver_enqueue_epochs: invalid argument");
    return SGDNET_EINVAL;
  }
  SGD_HIP_TRY(hipSetDevice(s->device));
  int rc = begin_batched_epochs(s, batch, stream_offset, draws_per_epoch * n_epochs, draws_per_epoch, n_epochs, &batch);
  if (rc) return rc;
  rc = ensure_graph(s, batch, draws_per_epoch);
  if (rc) return rc;
  const int nb = n_batches(batch, draws_per_epoch);
  for (int e = 0; e < n_epochs; ++e) {
    rc = launch_epoch(s, batch, draws_per_epoch);
    if (rc) return rc;
    lam_advance(s, draws_per_epoch, nb);
  }
  return SGDNET_OK;
}

int sgdnet_solver_sync(sgdnet_solver* s) {
  if (!s) return SGDNET_EINVAL;
  SGD_HIP_TRY(hipSetDevice(s->device));
  if (s->fused_in_graph && s->d.vsync) {        // epochs enqueued without a check of their own: did a fused launch give up?
    unsigned code = 0;
    SGD_HIP_TRY(hipMemcpyAsync(&code, s->d.vsync + vs_fused_sync_sticky_word(), sizeof(unsigned), hipMemcpyDeviceToHost, s->st));
    SGD_HIP_TRY(hipStreamSynchronize(s->st));
    if (code) {
      bool rerun = false;
      (void)fused_recover(s, 2, 0, 0, &rerun);
      drop_graph(s);
      set_error("batched mode: a fused epoch launch %s; the epochs enqueued since the last synchronisation are void "
                "(sgdnet_set_option(\"fused_epoch\", 0) keeps the separate launches)",
                code == 1 ? "could not become resident on the GPU (is it shared with another process?)"
                          : "timed out inside the epoch");
      return SGDNET_EHIP;
    }
  }
  SGD_HIP_TRY(hipStreamSynchronize(s->st));
  return check_bins(s);
}

int sgdnet_solver_profile_epoch(sgdnet_solver* s, int64_t batch, int64_t stream_offset,
                                int64_t draws_per_epoch, double* gather_ms, int* gather_launches,
                                double* sweep_ms, int* sweep_launches) {
  if (!s || draws_per_epoch <= 0 || !s->penalty_set) {
    set_error("sgdnet_solver_profile_epoch: invalid argument");
    return SGDNET_EINVAL;
  }
  SGD_HIP_TRY(hipSetDevice(s->device));
  int rc = begin_batched_epochs(s, batch, stream_offset, draws_per_epoch, draws_per_epoch, 1, &batch);
  if (rc) return rc;
  struct Events {                               // (registered before the launches they time: freed on every way out)
    std::vector<hipEvent_t> v;
    ~Events() {
      for (hipEvent_t e : v) (void)hipEventDestroy(e);
    }
  } events;
  std::vector<hipEvent_t>& ev = events.v;
#ifdef SGDNET_PHASE_TIMING
  const bool fused_prof = fused_epochs(s);
  if (fused_prof && s->d.dbg) SGD_HIP_TRY(hipMemsetAsync(s->d.dbg, 0, sizeof(unsigned long long) * 16 * 1024, s->st));
#endif
  rc = enqueue_epoch_kernels(s, batch, draws_per_epoch, &ev);
  if (rc) return rc;
  SGD_HIP_TRY(hipStreamSynchronize(s->st));
  lam_advance(s, draws_per_epoch, n_batches(batch, draws_per_epoch));
  double g = 0.0, w = 0.0;
  int ng = 0;
  for (size_t i = 0; i + 3 < ev.size(); i += 4) {
    float ms = 0.f;
    SGD_HIP_TRY(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
    g += ms;
    SGD_HIP_TRY(hipEventElapsedTime(&ms, ev[i + 2], ev[i + 3]));
    w += ms;
    ++ng;
  }
#ifdef SGDNET_PHASE_TIMING
  rc = phase_report_batched(s, batch, fused_prof);
  if (rc) return rc;
#endif
  if (gather_ms) *gather_ms = g;
  if (gather_launches) *gather_launches = ng;
  if (sweep_ms) *sweep_ms = w;
  if (sweep_launches) *sweep_launches = ng;
  return SGDNET_OK;
}

int sgdnet_solver_gather_form(const sgdnet_solver* s, int64_t batch) {
  if (!s || batch < 1) return 0;
  const BatchPlan g = plan(s, batch, batch);
  if (g.form == BatchForm::kFusedEpoch) return 3;
  if (g.form == BatchForm::kBinned) return 2;
  if (g.form == BatchForm::kShards) {
    // (kept from before the plan: the answer for the same solver without shards, whatever the shards launch)
    SagaDev d = s->d;
    d.V = 0;
    return plan_batch(d, (int)batch, PlanInputs{batch, s->bin_disabled, false, s->cus}).slab_doubles > 0 ? 1 : 0;
  }
  return g.slab_doubles > 0 ? 1 : 0;
}

int sgdnet_solver_last_change(const sgdnet_solver* s, double* max_change, double* max_size) {
  if (!s || !max_change || !max_size) return SGDNET_EINVAL;
  *max_change = s->last_change;
  *max_size = s->last_size;
  return SGDNET_OK;
}

int sgdnet_solver_epoch_timing(sgdnet_solver* s, int enable, double* sum_ms, int* launches) {
  if (!s) return SGDNET_EINVAL;
  SGD_HIP_TRY(hipSetDevice(s->device));
  SGD_HIP_TRY(hipStreamSynchronize(s->st));
  double tot = 0.0;
  int cnt = 0;
  for (size_t i = 0; i + 1 < s->epoch_ev.size(); i += 2) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, s->epoch_ev[i], s->epoch_ev[i + 1]) == hipSuccess) {
      tot += ms;
      ++cnt;
    }
  }
  for (hipEvent_t e : s->epoch_ev) s->ev_pool.push_back(e);   // (the stream is idle: every one of them has completed)
  s->epoch_ev.clear();
  s->time_epochs = enable != 0;
  if (enable) {
    const int rcp = fill_event_pool(s);
    if (rcp) return rcp;
  }
  if (sum_ms) *sum_ms = tot;
  if (launches) *launches = cnt;
  return SGDNET_OK;
}

int sgdnet_solver_convergence(sgdnet_solver* s, double tol, int* converged) {
  if (!s || !converged) return SGDNET_EINVAL;
  SGD_HIP_TRY(hipSetDevice(s->device));
  return device_convergence(s, tol, converged);
}

int64_t sgdnet_solver_sync_buffer_len(const sgdnet_solver* s) {
  if (!s) return 0;
  return (int64_t)s->d.K * s->d.p + 2 * 256 * (int64_t)s->d.K;
}

int sgdnet_solver_sync_bind(sgdnet_solver* s, void* device_buf) {
  if (!s) return SGDNET_EINVAL;
  SGD_HIP_TRY(hipSetDevice(s->device));
  SGD_HIP_TRY(hipStreamSynchronize(s->st));
  drop_graph(s);
  if (device_buf) {
    int rc = check_batched_ok(s);
    if (rc) return rc;
    if (!s->sparse) {
      set_error("the synchronous sharded mode is implemented for sparse x");
      return SGDNET_EUNSUPPORTED;
    }
    if (!s->own_D) {
      s->own_D = s->d.D;
      s->own_d0 = s->d.d0_part;
    }
    double* buf = static_cast<double*>(device_buf);
    SGD_HIP_TRY(hipMemsetAsync(buf, 0, sizeof(double) * (size_t)sgdnet_solver_sync_buffer_len(s), s->st));
    s->d.D = buf;
    s->d.d0_part = buf + (int64_t)s->d.K * s->d.p;
    s->d.force_global = 1;
  } else if (s->own_D) {
    s->d.D = s->own_D;
    s->d.d0_part = s->own_d0;
    s->own_D = s->own_d0 = nullptr;
    s->d.force_global = 0;
  }
  SGD_HIP_TRY(hipStreamSynchronize(s->st));
  return SGDNET_OK;
}

int sgdnet_solver_sync_begin(sgdnet_solver* s, int64_t stream_offset, int64_t draws_local_per_epoch) {
  if (!s || !s->penalty_set || !s->d.force_global || draws_local_per_epoch <= 0) {
    set_error("sgdnet_solver_sync_begin: bind a sync buffer and set the penalty first");
    return SGDNET_EINVAL;
  }
  SGD_HIP_TRY(hipSetDevice(s->device));
  int rc = check_stream(s, stream_offset, draws_local_per_epoch);
  if (rc) return rc;
  s->lam.stream_base = stream_offset;
  s->lam.stream_wrap = 0;
  s->lam.draws_per_epoch = draws_local_per_epoch;
  rc = push_lam(s);
  if (rc) return rc;
  if (s->d.standardize) rc = launch_cw_init(s->d, s->lam_dev, s->st);
  return rc;
}

int sgdnet_solver_sync_gather(sgdnet_solver* s, int64_t t0_local, int64_t m_local, int round) {
  if (!s || !s->d.force_global || t0_local < 0 || m_local < 0) return SGDNET_EINVAL;
  if (m_local == 0) return SGDNET_OK;
  SGD_HIP_TRY(hipSetDevice(s->device));
  return launch_batch_gather(s->d, plan(s, m_local, m_local), s->lam_dev, t0_local, (int)m_local, round, s->st);
}

int sgdnet_solver_sync_sweep(sgdnet_solver* s, int64_t m_global, int64_t m_local, int round) {
  if (!s || !s->d.force_global || m_global <= 0) return SGDNET_EINVAL;
  SGD_HIP_TRY(hipSetDevice(s->device));
  double r_m, ls_m;
  batch_factors(s->lam.alpha, s->lam.gamma, m_global, &r_m, &ls_m);
  const int64_t m = m_local > 0 ? m_local : 1;
  return launch_batch_sweep(s->d, plan(s, m, m), s->lam_dev, s->lam.penalty, 0, round, s->st, nullptr, nullptr, r_m, ls_m,
                            (double)m_global);
}

int sgdnet_solver_sync_end(sgdnet_solver* s, int rounds) {
  if (!s || rounds <= 0) return SGDNET_EINVAL;
  SGD_HIP_TRY(hipSetDevice(s->device));
  int rc = launch_epoch_end(s->lam_dev, rounds, s->st);
  if (rc) return rc;
  lam_advance(s, s->lam.draws_per_epoch, rounds);   // mirrors end_epoch on the device
  return SGDNET_OK;
}

}  // extern "C"
