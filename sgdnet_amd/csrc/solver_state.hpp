// The solver behind the sgdnet_solver_* C ABI (include/sgdnet_hip.h) as its own translation units see it:
//   solver.cpp         life cycle and data: create / destroy, options, records, binned scratch, state, deltas
//   solver_epoch.cpp   everything that enqueues an epoch: the LamParams mirror, the plan, the graph cache, the entry points
//   solver_rng.cpp     the stream buffer and the sample-order pipeline (the only writer of RngPipe::raw / pending_gen)
//   solver_shards.cpp  virtual shards, and the links between solvers (peer access, IPC)
//   phase_report.cpp   the printouts of SGDNET_PHASE_TIMING builds
// Private to those files.  driver.cpp and the kernels' files know the solver through common.hpp, setup_device.hpp and
// the C ABI only.
#pragma once

#include <vector>

#include "common.hpp"
#include "setup_device.hpp"

struct sgdnet_solver {
  sgdnet::SagaDev d{};
  bool sparse = false;
  int device = 0;
  hipStream_t st = nullptr;
  sgdnet::LamParams lam{};
  sgdnet::LamParams* lam_dev = nullptr;
  sgdnet::LamParams lam_dev_mirror{};   // what lam_dev holds (push_lam skips an upload that would change nothing)
  bool lam_dev_valid = false;
  // pinned staging ring for the asynchronous upload of `lam`: the host copy keeps changing
  // (stream_base, batch_seq) while earlier uploads may still be in flight
  static constexpr int kLamSlots = 8;
  sgdnet::LamParams* lam_stage = nullptr;
  hipEvent_t lam_ev[kLamSlots] = {};
  int lam_slot = 0;
  // owned device buffers
  std::vector<void*> owned;
  double* ref = nullptr;        // snapshot for the multi-GPU merge
  double* LS_dev = nullptr;     // lag_scaling table (exact sparse)
  int64_t LS_len = 0;
  double LS_alpha = -1.0, LS_gamma = -1.0;
  int* out_dev = nullptr;
  uint32_t* stream_dev = nullptr;
  int64_t stream_len = 0;
  int64_t stream_cap = 0;
  uint32_t* rng_dev = nullptr;  // 625 words: the device copy of a sgdnet_rng
  // sample-order pipeline of the fit driver (solver_rng_*): the next epoch's draws are
  // generated on a side stream while the current epoch runs
  struct RngPipe {
    bool open = false;
    hipStream_t st = nullptr;
    hipEvent_t ready[2] = {nullptr, nullptr};   // slot filled (side stream)
    hipEvent_t freed[2] = {nullptr, nullptr};   // slot consumed (solver stream)
    uint32_t* state[2] = {nullptr, nullptr};    // generation g reads state[g & 1], writes state[(g + 1) & 1]
    int64_t n = 0;
    int64_t gens = 0, used = 0;
    static constexpr int kMaxGen = 64;
    int G = 1;                                  // generators side by side (segments of an epoch's stream)
    // G > 1: ONE R stream.  state[.][g] is the state at the START of generator g's segment;
    // the next epoch's starts are those states jumped n draws ahead (poly_n), the ends the generation
    // kernel leaves go to `ends` and are not used
    uint32_t* poly_n = nullptr;
    uint32_t* ends = nullptr;
    int64_t run_len = 0;   // virtual shards: draws per run of the layout (0: one run = the epoch)
    // what the slot's memory holds (in stream order): the generators' raw words, or draws.  Raw slots are left to the
    // fused epoch kernel, which turns a word into a draw where it reads it and writes nothing back: a slot it has
    // consumed is still raw.  Every other reader goes through slot_to_draws() first, the ONLY place that clears this
    // (solver_rng.cpp: no other file assigns raw[] or pending_gen).
    bool raw[2] = {false, false};
    // generators inside the fused epoch kernel (SagaDev::rngdev): the generation that the next fused launch is to
    // produce, or -1; a generation still pending when its draws are asked for is produced on the side stream after all
    sgdnet::RngDev* dev = nullptr;
    int64_t pending_gen = -1;
    // Steady state of the fused epochs: the launch of epoch e reads slot e & 1, which the launch of epoch e - 1 filled
    // (in_kernel[]), and fills the other slot itself.  Producer and consumer are consecutive kernels of the solver's
    // stream, the side stream is idle, and nothing but the kernel is enqueued: no wait for ready[], no record of
    // freed[] (`quiet`, decided per launch in prepare_stream_slot).  The record is owed instead (freed_owed[]).
    // INVARIANT: the side stream never writes a slot, or a generator state, that an enqueued launch still reads.
    // Every write of the side stream goes through rng_side_generate(), which first waits for freed[slot]; if that
    // record is owed it is made there, on the solver's stream behind everything enqueued so far.  solver_rng.cpp
    // stays the only file that assigns raw[], pending_gen and these flags.
    bool in_kernel[2] = {false, false};         // the slot's content comes from a fused launch on the solver's stream
    bool freed_owed[2] = {false, false};        // a launch read the slot and no freed[] record stands behind it yet
    bool quiet = false;                         // the launch being enqueued needs no marker on either side
  } pipe;
  int64_t nnz = 0;
  bool penalty_set = false;
  // cached epoch graph
  // captured epochs, one per (batch, draws) shape; gexec is the one selected by ensure_graph
  struct GraphEntry {
    int64_t batch, draws;
    hipGraph_t graph;
    hipGraphExec_t exec;
    int fused;                  // > 0: the epoch is ONE launch of saga_vs_epoch_kernel (the value of option fused_epoch)
  };
  std::vector<GraphEntry> graphs;
  hipGraphExec_t gexec = nullptr;
  bool w_prev_valid = false;
  double last_change = 0.0, last_size = 0.0;
  int64_t slab_cap = 0;         // doubles the slab buffer can hold
  double* own_D = nullptr;      // the solver's own D / d0 slots while a sync buffer is bound
  std::vector<void*> vs_owned;  // virtual-shard replicas
  int64_t vs_period = 0;        // draws per shard between device-side merges (0: n / 32)
  double* own_d0 = nullptr;
  // binned form (batched_binned.hip): ranges built once, bins sized for the current batch
  bool bin_ranges_ready = false;
  int64_t bin_batch = 0;        // the batch the bins and gcb were sized for
  void* bin_bufs[3] = {nullptr, nullptr, nullptr};   // bins, gcb, bin_off
  std::vector<double> bin_mass;  // non-zeros of every feature range
  std::vector<double> bin_sumsq; // sum over samples of (its non-zeros inside the range)^2
  double bin_slack = 8.0, bin_slack_built = 0.0;   // standard deviations of room in every bin
  bool bin_disabled = false;     // a bin kept overflowing: the solver runs the atomic form (K <= 16) from now on
  bool bin_overflowed = false;   // the last sync found an overflow (the epochs since the previous sync are void)
  // one-response sparse fits with compact records: the batched kernels keep the gradient memory inside the
  // records (batched_k1.hpp "Compact records"), everything else (exact mode, the host) sees the K x n array
  bool m_in_rec = false;
  // fused epoch of the virtual shards (saga_vs_epoch_kernel): switched off for this solver once a launch could not
  // become resident (a GPU shared with another process); the separate launches take over
  bool fused_off = false;
  int cus = 0;                   // the device's compute units (read once: the fused epoch needs one workgroup per CU)
  bool fused_in_graph = false;   // the captured epochs use it
  int fused_abort_seen = 0;      // LamParams::fused_abort as the last ConvergenceCheck read it
  sgdnet::FusedPeers* peers_dev = nullptr;   // sgdnet_solver_link_peers
  // sgdnet_solver_epoch_timing: dispatch start / stop events of every fused epoch launch (the benchmark's timed region)
  bool time_epochs = false;
  std::vector<hipEvent_t> epoch_ev;
  std::vector<hipEvent_t> ev_pool;   // events of earlier timed regions, reused: none is created while a timed region runs
  std::vector<void*> ipc_opened;   // sgdnet_solver_link_ipc: the peers' buffers as mapped here
  // SGDNET_TRACE: host-side split of this solver's batched epochs (development aid; sgdnet_solver_destroy prints it).
  // The events bracket an epoch's launch on the solver's stream: created on first use, on the solver's device.
  hipEvent_t trace_ev[2] = {nullptr, nullptr};
  double trace_launch = 0.0, trace_conv = 0.0, trace_graph = 0.0;
  long trace_epochs = 0;
};

// The helpers that cross the units' boundaries.  (Hidden: the library exports what it exported as one file.)
#pragma GCC visibility push(hidden)
namespace sgdnet {

// solver.cpp
int m_to_record(sgdnet_solver* s);
int m_to_array(sgdnet_solver* s);
int ensure_binned(sgdnet_solver* s, int64_t batch);
int ensure_dense_tiled(sgdnet_solver* s, int64_t batch);

// solver_epoch.cpp
void drop_graph(sgdnet_solver* s);
int push_lam(sgdnet_solver* s);
BatchPlan plan(const sgdnet_solver* s, int64_t batch, int64_t m);
bool fused_epochs(const sgdnet_solver* s);
int device_loss_sum(sgdnet_solver* s, double* out);

// solver_rng.cpp
int64_t stream_wrap_for(const sgdnet_solver* s, int64_t stream_offset, int64_t draws);
int stream_to_draws(sgdnet_solver* s, int64_t offset, int64_t count);
int prepare_stream_slot(sgdnet_solver* s, int64_t batch, int64_t stream_offset, int64_t draws, int n_epochs);

#ifdef SGDNET_PHASE_TIMING
// phase_report.cpp
int phase_report_exact(const sgdnet_solver* s, const ExactPlan& plan, int epochs, int64_t draws_per_epoch);
int phase_report_batched(const sgdnet_solver* s, int64_t batch, bool fused_prof);
#endif

}  // namespace sgdnet
#pragma GCC visibility pop
