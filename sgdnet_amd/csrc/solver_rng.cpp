// The solver's sample stream (solver_state.hpp): the resident stream buffer -- uploaded, generated on the device or
// read back -- and the sample-order pipeline of the fit driver, which generates the next epoch's draws while the
// current epoch runs (solver_rng_open / prefetch / acquire / release / close and their sgdnet_solver_rng_* wrappers).
// What a slot of the pipeline holds, raw words or draws (RngPipe::raw[]), and which generation is still owed
// (RngPipe::pending_gen) are assigned in this file and nowhere else; slot_to_draws() is the one place that converts a
// slot and clears its flag.  The same holds for the flags that let back-to-back fused epochs go without stream markers
// (RngPipe::in_kernel / freed_owed / quiet, and the invariant stated beside them).
#include <algorithm>
#include <vector>

#include "solver_state.hpp"

namespace sgdnet {

// Epochs that consume the sample-order pipeline's two-epoch buffer alternate between its halves: the device
// wraps stream_base there itself, so consecutive epochs need no upload.
int64_t stream_wrap_for(const sgdnet_solver* s, int64_t stream_offset, int64_t draws) {
  const auto& P = s->pipe;
  return (P.open && draws == P.n && (stream_offset == 0 || stream_offset == P.n)) ? 2 * P.n : 0;
}

// Slot q of the sample-order pipeline: raw words -> draws, in place, on the solver's stream, if it holds raw words.
// The conversion is not idempotent; the slot's flag is tested and cleared here and nowhere else.
static int slot_to_draws(sgdnet_solver* s, int q) {
  auto& P = s->pipe;
  if (!P.raw[q]) return SGDNET_OK;
  SGD_HIP_TRY(hipStreamWaitEvent(s->st, P.ready[q], 0));        // a generation on the side stream (none: no wait)
  int rc = launch_rng_convert(s->stream_dev + (int64_t)q * P.n, P.n, (uint32_t)s->d.n, s->st, s->d.V, s->d.v_size,
                              P.run_len);
  if (rc) return rc;
  P.raw[q] = false;
  return SGDNET_OK;
}

// entries [offset, offset + count) of the stream are about to be read as draws by something that is not the fused
// epoch kernel
int stream_to_draws(sgdnet_solver* s, int64_t offset, int64_t count) {
  auto& P = s->pipe;
  if (!P.open || !(P.raw[0] || P.raw[1])) return SGDNET_OK;
  for (int q = 0; q < 2; ++q) {
    if (offset >= (int64_t)(q + 1) * P.n || offset + count <= (int64_t)q * P.n) continue;
    int rc = slot_to_draws(s, q);
    if (rc) return rc;
  }
  return SGDNET_OK;
}

// The epoch(s) about to be enqueued read the stream at `stream_offset`.  A slot of the sample-order pipeline that was
// left raw goes to the fused epoch kernel as it is (LamParams::stream_raw) and stays raw: the kernel only reads it.
// For any other consumer it is converted now, on the solver's stream.
int prepare_stream_slot(sgdnet_solver* s, int64_t batch, int64_t stream_offset, int64_t draws, int n_epochs) {
  auto& P = s->pipe;
  s->lam.stream_raw = 0;
  s->lam.rng_generate = 0;
  P.quiet = false;
  if (!P.open) return SGDNET_OK;
  const bool one_slot = n_epochs == 1 && draws == P.n && (stream_offset == 0 || stream_offset == P.n);
  const int slot = stream_offset == 0 ? 0 : 1;
  const bool fused = one_slot && plan(s, batch, batch).form == BatchForm::kFusedEpoch;
  // the launch that consumes generation `used` also produces the pending generation used + 1 (its spare workgroups)
  if (fused && s->d.rngdev && P.pending_gen >= 0 && P.pending_gen == P.used + 1 && slot == (int)(P.used & 1)) {
    s->lam.rng_generate = 1;
    P.raw[P.pending_gen & 1] = true;            // (the other slot: raw words from this launch on)
    P.in_kernel[P.pending_gen & 1] = true;
    P.pending_gen = -1;
  }
  if (!(P.raw[0] || P.raw[1])) return SGDNET_OK;
  if (fused && P.raw[slot]) {
    s->lam.stream_raw = 1;
    // produced by the launch before, the next generation inside this one: the side stream has no part in this epoch
    P.quiet = s->lam.rng_generate != 0 && P.in_kernel[slot] && P.run_len == 0;
    return SGDNET_OK;
  }
  for (int q = 0; q < 2; ++q) {
    if (!P.raw[q] || (one_slot && q != slot)) continue;
    if (!one_slot) SGD_HIP_TRY(hipStreamSynchronize(P.st));      // a slot that may still be generated
    int rc = slot_to_draws(s, q);
    if (rc) return rc;
  }
  return SGDNET_OK;
}

static int reserve_stream(sgdnet_solver* s, int64_t count) {
  if (count > s->stream_cap || !s->stream_dev) {
    SGD_HIP_TRY(hipStreamSynchronize(s->st));
    if (s->stream_dev) SGD_HIP_TRY(hipFree(s->stream_dev));
    s->stream_dev = nullptr;
    SGD_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&s->stream_dev), sizeof(uint32_t) * (size_t)count));
    s->stream_cap = count;
    drop_graph(s);  // captured kernels hold the old pointer
  }
  s->stream_len = count;
  s->d.stream = s->stream_dev;
  return SGDNET_OK;
}

}  // namespace sgdnet

using namespace sgdnet;

// ---- sample-order pipeline (driver.cpp) -------------------------------------------------------
// The stream buffer holds two epochs; epoch e reads half e & 1 while the side stream fills the
// other half with the draws of epoch e + 1.  The generator state ping-pongs between two device
// buffers, so the state after exactly `used` epochs survives one speculative generation.
// generators > 1 (batched mode, where the trajectory is not the reference's anyway): the epoch's
// stream is cut into that many consecutive segments, each filled by its own MT19937 -- the
// caller's generator for segment 0, and for segment g a generator seeded (set.seed scrambling,
// r_rng.cpp) with floor(2^32 * unif_rand()) drawn from the caller's generator at this point.
// One generator makes 10M draws in 5.3 ms, which is six epochs of the batched kernels at C4.
// jump_draws: draws of the WHOLE job per epoch when this solver holds one rank's range of a stream shared by several
// (driver.cpp, control.n_gpus); 0: n
int solver_rng_open(sgdnet_solver* s, sgdnet_rng* rng, int64_t n, int generators, int64_t jump_draws) {
  SGD_HIP_TRY(hipSetDevice(s->device));
  auto& P = s->pipe;
  if (generators < 1) generators = 1;
  if (generators > sgdnet_solver::RngPipe::kMaxGen) generators = sgdnet_solver::RngPipe::kMaxGen;
  int rc = reserve_stream(s, 2 * n);
  if (rc) return rc;
  if (!P.st) {
    SGD_HIP_TRY(hipStreamCreateWithFlags(&P.st, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
      SGD_HIP_TRY(hipEventCreateWithFlags(&P.ready[i], hipEventDisableTiming));
      SGD_HIP_TRY(hipEventCreateWithFlags(&P.freed[i], hipEventDisableTiming));
      SGD_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&P.state[i]),
                            sizeof(sgdnet_rng) * sgdnet_solver::RngPipe::kMaxGen));
    }
  }
  // Several generators work on ONE stream -- R's, as set.seed() left it: generator g starts
  // g * seg draws into the epoch (its state = the first one jumped g * seg draws ahead), and every
  // epoch all starts move n draws on (mt_jump.cpp).  If the jump polynomials cannot be had the fit
  // keeps a single generator.
  const int64_t seg = (n + generators - 1) / generators;
  std::vector<uint32_t> poly_seg(624), poly_n(624);
  if (generators > 1 && !(mt_jump_poly((uint64_t)seg, poly_seg.data()) &&
                          mt_jump_poly((uint64_t)(jump_draws > 0 ? jump_draws : n), poly_n.data())))
    generators = 1;
  P.G = generators;
  {
    // the generators' workgroups get CUs of their own: the LDS gather forms shrink their grids
    // one workgroup per generator up to 8 workgroups, then up to four generators per workgroup: the generators' work
    // per epoch (state step: seg / 624 blocks of ~0.46 us; jump: ~64 us per generator and workgroup) must stay below the
    // epoch's own duration -- at C3 (1M draws, 8 generators) two workgroups of four needed 370 us beside a 246-us epoch
    const int per_wg = rng_generators_per_workgroup();
    const int reserve = generators > 1 ? std::max(std::min(generators, 8), (generators + per_wg - 1) / per_wg) : 0;
    // (Tried: confining the side stream to exactly those CUs with hipExtStreamCreateWithCUMask -- mask bit i is a
    // CU of XCC i % 8, scripts/microbench/cu_mask.hip -- so that the conversion kernel's 2048 small workgroups
    // cannot spread over CUs a gather launch is about to need: on 8 CUs that kernel takes 0.8 ms instead of 0.05,
    // the side stream becomes the epoch's critical path (1.32 ms per epoch) and the gather beside it is slower,
    // not faster (90 us per launch).  A masked stream for the solver itself places N whole-LDS workgroups on
    // N - 1 of its N CUs, i.e. runs two rounds.  profiles/r03p_cu_mask_microbench.txt, r03q_*.)
    if (reserve != s->d.cu_reserve) {
      SGD_HIP_TRY(hipStreamSynchronize(s->st));
      s->d.cu_reserve = reserve;
      if (s->d.V > 1) s->d.v_bps = lds_target_grid(s->d) / s->d.V;
      drop_graph(s);
    }
  }
  SGD_HIP_TRY(hipMemcpy(P.state[0], rng, sizeof(sgdnet_rng), hipMemcpyHostToDevice));
  if (generators > 1) {
    if (!P.poly_n) {
      SGD_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&P.poly_n), sizeof(uint32_t) * 624 * 2));
      SGD_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&P.ends), sizeof(sgdnet_rng) * sgdnet_solver::RngPipe::kMaxGen));
    }
    SGD_HIP_TRY(hipMemcpy(P.poly_n, poly_n.data(), sizeof(uint32_t) * 624, hipMemcpyHostToDevice));
    SGD_HIP_TRY(hipMemcpy(P.poly_n + 624, poly_seg.data(), sizeof(uint32_t) * 624, hipMemcpyHostToDevice));
    for (int g = 1; g < generators; ++g) {      // start[g] = start[g - 1] jumped seg draws: once per fit
      int rcj = launch_rng_jump(P.state[0] + (size_t)(g - 1) * 625, P.state[0] + (size_t)g * 625, P.poly_n + 624, 1, P.st);
      if (rcj) return rcj;
    }
    SGD_HIP_TRY(hipStreamSynchronize(P.st));
  }
  SGD_HIP_TRY(hipStreamSynchronize(s->st));
  for (int i = 0; i < 2; ++i) SGD_HIP_TRY(hipEventRecord(P.freed[i], s->st));
  P.n = n;
  P.gens = P.used = 0;
  P.pending_gen = -1;
  P.raw[0] = P.raw[1] = false;
  P.in_kernel[0] = P.in_kernel[1] = false;
  P.freed_owed[0] = P.freed_owed[1] = false;    // (recorded just above)
  P.quiet = false;
  // the same generators as the fused epoch kernel of the virtual shards runs them on its spare workgroups
  RngDev* want = nullptr;
  if (generators > 1 && s->d.V > 1 && s->d.vsync) {
    if (!P.dev) SGD_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&P.dev), sizeof(RngDev)));
    RngDev h{};
    h.state[0] = P.state[0];
    h.state[1] = P.state[1];
    h.ends = P.ends;
    h.stream = s->stream_dev;
    h.poly = P.poly_n;
    h.n = n;
    h.seg = seg;
    h.gens = generators;
    h.gen = 0u;
    SGD_HIP_TRY(hipMemcpy(P.dev, &h, sizeof(RngDev), hipMemcpyHostToDevice));
    want = P.dev;
  }
  if (want != s->d.rngdev) {
    s->d.rngdev = want;
    drop_graph(s);
  }
  P.open = true;
  return SGDNET_OK;
}

// generation g of the sample order on the side stream: slot g & 1, start states state[g & 1] -> state[(g + 1) & 1]
static int rng_side_generate(sgdnet_solver* s, int64_t g, bool keep_raw) {
  auto& P = s->pipe;
  const int slot = (int)(g & 1);
  // Launches that went without their record (solver_rng_release) are covered here: behind everything enqueued so far,
  // which is also behind the fused launch that left the start states state[g & 1] (it precedes the slot's last reader).
  if (P.freed_owed[slot]) {
    SGD_HIP_TRY(hipEventRecord(P.freed[slot], s->st));
    P.freed_owed[slot] = false;
  }
  SGD_HIP_TRY(hipStreamWaitEvent(P.st, P.freed[slot], 0));
  int rc;
  P.raw[slot] = keep_raw;
  P.in_kernel[slot] = false;
  if (P.G > 1) {
    rc = launch_rng_fill(P.state[g & 1], P.ends, (uint32_t)s->d.n, s->stream_dev + (int64_t)slot * P.n, P.n,
                         P.st, s->d.V, s->d.v_size, P.G, P.run_len, keep_raw ? 0 : 1, 0, s->d.cu_reserve);
    // the jump's workgroups take their generators in turn: the side stream never holds more CUs than
    // the generators' own (a wider launch would push gather workgroups into a second round)
    if (!rc) rc = launch_rng_jump(P.state[g & 1], P.state[(g + 1) & 1], P.poly_n, P.G, P.st,
                                  std::max(1, s->d.cu_reserve));
  } else {
    rc = launch_rng_fill(P.state[g & 1], P.state[(g + 1) & 1], (uint32_t)s->d.n,
                         s->stream_dev + (int64_t)slot * P.n, P.n, P.st, s->d.V, s->d.v_size, P.G, P.run_len,
                         keep_raw ? 0 : 1);
  }
  if (rc) return rc;
  if (P.dev)                                    // the in-kernel generators continue from here
    SGD_HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(&P.dev->gen), (int)(g + 1), 1, P.st));
  SGD_HIP_TRY(hipEventRecord(P.ready[slot], P.st));
  return SGDNET_OK;
}

// enqueue the next generation (never more than one ahead of the epoch being consumed)
int solver_rng_prefetch(sgdnet_solver* s) {
  auto& P = s->pipe;
  if (!P.open || P.gens > P.used + 1) return SGDNET_EINVAL;
  SGD_HIP_TRY(hipSetDevice(s->device));
  // Virtual shards with the fused epoch kernel: that kernel holds every CU for a whole epoch, so its own spare
  // workgroups produce the next generation (raw words: the NEXT epoch's launch turns them into draws as it reads
  // them), and nothing is launched here: the generation is pending until the launch that carries it is enqueued
  // (prepare_stream_slot), or until its draws are asked for without such a launch (solver_rng_acquire).
  // (Generators launched beside the epoch kernel raced it for CUs: dispatched together, one epoch workgroup per XCD
  //  found its CU taken and the whole epoch waited for the generators, +215 us; dispatched later, their own
  //  workgroups could stall until the epoch ended -- profiles/r04_rng_placement.txt.)
  const bool keep_raw = P.run_len == 0 && fused_epochs(s);
  if (keep_raw && P.dev && s->d.rngdev && P.G > 1 && P.gens >= 1 && P.pending_gen < 0) {
    P.pending_gen = P.gens;                     // (its slot keeps what it holds, and its flag, until then)
    ++P.gens;
    return SGDNET_OK;
  }
  int rc = rng_side_generate(s, P.gens, keep_raw);
  if (rc) return rc;
  ++P.gens;
  return SGDNET_OK;
}

// the solver's stream waits for the draws of the next unconsumed epoch; *offset = where they are
int solver_rng_acquire(sgdnet_solver* s, int64_t* offset) {
  auto& P = s->pipe;
  if (!P.open || P.gens <= P.used) return SGDNET_EINVAL;
  const int slot = (int)(P.used & 1);
  if (P.pending_gen == P.used) {                // no fused launch carried this generation: the side stream makes it now
    const int64_t g = P.pending_gen;
    P.pending_gen = -1;
    SGD_HIP_TRY(hipEventRecord(P.freed[slot], s->st));       // after everything enqueued so far
    P.freed_owed[slot] = false;
    int rc = rng_side_generate(s, g, true);     // (a generation is only ever pending as raw words)
    if (rc) return rc;
  }
  // a slot that a fused launch filled needs no wait: that launch precedes every reader on the solver's stream
  if (!P.in_kernel[slot]) SGD_HIP_TRY(hipStreamWaitEvent(s->st, P.ready[slot], 0));
  *offset = (int64_t)slot * P.n;
  return SGDNET_OK;
}

// the epoch that consumed the acquired draws has been enqueued on the solver's stream
int solver_rng_release(sgdnet_solver* s) {
  auto& P = s->pipe;
  const int slot = (int)(P.used & 1);
  if (P.quiet) {                                // nothing but the kernel between two fused epochs: the record is owed
    P.freed_owed[slot] = true;                  // (rng_side_generate makes it before the side stream touches the slot)
    P.quiet = false;
  } else {
    SGD_HIP_TRY(hipEventRecord(P.freed[slot], s->st));
    P.freed_owed[slot] = false;
  }
  ++P.used;
  return SGDNET_OK;
}

// generator state after exactly `used` epochs (a speculative generation is discarded)
int solver_rng_close(sgdnet_solver* s, sgdnet_rng* rng) {
  auto& P = s->pipe;
  if (!P.open) return SGDNET_OK;
  SGD_HIP_TRY(hipSetDevice(s->device));
  if (P.pending_gen >= 0) {                     // a generation nobody produced: it does not exist (the state below is
    --P.gens;                                   // the one after `used` epochs either way)
    P.pending_gen = -1;
  }
  SGD_HIP_TRY(hipStreamSynchronize(P.st));
  SGD_HIP_TRY(hipStreamSynchronize(s->st));
  SGD_HIP_TRY(hipMemcpy(rng, P.state[P.used & 1], sizeof(sgdnet_rng), hipMemcpyDeviceToHost));
  for (int q = 0; q < 2; ++q) {                 // slots the fused epoch kernel consumed, or never got to: draws from here on
    int rcq = slot_to_draws(s, q);
    if (rcq) return rcq;
  }
  P.open = false;
  if (s->d.rngdev) {
    s->d.rngdev = nullptr;
    drop_graph(s);
  }
  if (s->d.cu_reserve) {
    s->d.cu_reserve = 0;
    if (s->d.V > 1) s->d.v_bps = lds_target_grid(s->d) / s->d.V;
    drop_graph(s);
  }
  return SGDNET_OK;
}

extern "C" {

int sgdnet_solver_upload_stream(sgdnet_solver* s, const uint32_t* host, int64_t count) {
  if (!s || !host || count <= 0) {
    set_error("sgdnet_solver_upload_stream: invalid argument");
    return SGDNET_EINVAL;
  }
  // the kernels use the entries as addresses (ptr[s + 1], g_memory[s * K]): reject anything
  // that is not a sample index before it reaches the device
  uint32_t top = 0;
  for (int64_t i = 0; i < count; ++i) top = host[i] > top ? host[i] : top;
  if ((int64_t)top >= s->d.n) {
    set_error("sgdnet_solver_upload_stream: entry %u is not a sample index (n_samples = %lld)", top,
              (long long)s->d.n);
    return SGDNET_EINVAL;
  }
  SGD_HIP_TRY(hipSetDevice(s->device));
  int rc = reserve_stream(s, count);
  if (rc) return rc;
  SGD_HIP_TRY(hipMemcpyAsync(s->stream_dev, host, sizeof(uint32_t) * (size_t)count, hipMemcpyHostToDevice,
                             s->st));
  SGD_HIP_TRY(hipStreamSynchronize(s->st));
  return SGDNET_OK;
}

int sgdnet_solver_get_stream(sgdnet_solver* s, uint32_t* host, int64_t offset, int64_t count) {
  if (!s || !host || offset < 0 || count <= 0 || offset + count > s->stream_len) {
    set_error("sgdnet_solver_get_stream: range outside the resident stream");
    return SGDNET_EINVAL;
  }
  SGD_HIP_TRY(hipSetDevice(s->device));
  int rc = stream_to_draws(s, offset, count);   // a slot left raw (also one a fused epoch has consumed) reads back as draws
  if (rc) return rc;
  SGD_HIP_TRY(hipMemcpyAsync(host, s->stream_dev + offset, sizeof(uint32_t) * (size_t)count,
                             hipMemcpyDeviceToHost, s->st));
  SGD_HIP_TRY(hipStreamSynchronize(s->st));
  return SGDNET_OK;
}

int sgdnet_solver_generate_stream(sgdnet_solver* s, sgdnet_rng* rng, int64_t count) {
  if (!s || !rng || count <= 0) {
    set_error("sgdnet_solver_generate_stream: invalid argument");
    return SGDNET_EINVAL;
  }
  SGD_HIP_TRY(hipSetDevice(s->device));
  int rc = reserve_stream(s, count);
  if (rc) return rc;
  if (!s->rng_dev) SGD_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&s->rng_dev), sizeof(sgdnet_rng)));
  static_assert(sizeof(sgdnet_rng) == 625 * sizeof(uint32_t), "sgdnet_rng is mti + 624 words");
  SGD_HIP_TRY(hipMemcpyAsync(s->rng_dev, rng, sizeof(sgdnet_rng), hipMemcpyHostToDevice, s->st));
  rc = launch_rng_fill(s->rng_dev, s->rng_dev, (uint32_t)s->d.n, s->stream_dev, count, s->st, s->d.V, s->d.v_size);
  if (rc) return rc;
  SGD_HIP_TRY(hipMemcpyAsync(rng, s->rng_dev, sizeof(sgdnet_rng), hipMemcpyDeviceToHost, s->st));
  SGD_HIP_TRY(hipStreamSynchronize(s->st));
  return SGDNET_OK;
}

// ---- sample-order pipeline in the C ABI (what sgdnet_fit_* uses internally) ----
int sgdnet_solver_rng_open(sgdnet_solver* s, sgdnet_rng* rng, int64_t draws_per_epoch, int generators) {
  if (!s || !rng || draws_per_epoch <= 0) {
    set_error("sgdnet_solver_rng_open: invalid argument");
    return SGDNET_EINVAL;
  }
  int rc = solver_rng_open(s, rng, draws_per_epoch, generators);
  if (rc) return rc;
  return solver_rng_prefetch(s);
}

int sgdnet_solver_rng_layout(sgdnet_solver* s, int64_t draws_per_run) {
  if (!s || draws_per_run < 0) return SGDNET_EINVAL;
  if (s->pipe.open) {
    set_error("sgdnet_solver_rng_layout: set the layout before sgdnet_solver_rng_open");
    return SGDNET_EINVAL;
  }
  s->pipe.run_len = draws_per_run;
  return SGDNET_OK;
}

int sgdnet_solver_rng_next(sgdnet_solver* s, int64_t* stream_offset) {
  if (!s || !stream_offset) return SGDNET_EINVAL;
  int rc = solver_rng_prefetch(s);               // the epoch after this one, concurrently
  if (rc) return rc;
  return solver_rng_acquire(s, stream_offset);
}

int sgdnet_solver_rng_done(sgdnet_solver* s) { return s ? solver_rng_release(s) : SGDNET_EINVAL; }

int sgdnet_solver_rng_close(sgdnet_solver* s, sgdnet_rng* rng) {
  if (!s || !rng) return SGDNET_EINVAL;
  return solver_rng_close(s, rng);
}

}  // extern "C"
