// Batched SAGA, host-visible geometry: the block sizes and LDS budgets that plan_batch (batched_plan.cpp) and the
// launchers of the kernel families (saga_batched.hip, batched_*.hip) both read, the one kernel launcher, and the
// per-family launchers behind the dispatching launch_batch_gather / launch_batch_sweep.
#pragma once

#include <hip/hip_ext.h>

#include <type_traits>

#include "common.hpp"

#ifndef SGDNET_BIN_BLOCK
#define SGDNET_BIN_BLOCK 1024
#endif
#ifndef SGDNET_BIN_W
#define SGDNET_BIN_W 8
#endif
#ifndef SGDNET_RANGE_BLOCK
#define SGDNET_RANGE_BLOCK 512
#endif
#ifndef SGDNET_LDS_BLOCK
#define SGDNET_LDS_BLOCK 1024
#endif

namespace sgdnet {

constexpr int kGroup = 16;          // lanes per draw
constexpr int kBlock = 256;

// Intercept accumulator d0[k] = sum_i gc_ik: two sets (batch parity) of kD0Slots slots.  A
// gather with at most kD0Slots workgroups stores one partial per workgroup; a larger grid adds
// atomically into slot (workgroup % kD0Slots) of a set the previous sweep left zeroed.  Either
// way the sweep sums at most kD0Slots values per class (thousands of same-address atomics, or
// thousands of partials summed by one block, would each cost tens of microseconds).
constexpr int kD0Slots = 256;

// what the eligibility rules read of the K == 1 record forms (batched_k1.hpp): bytes of a compact record, the bits of a
// tagged sample id that hold the id, and the entries of a row the 8-lane forms keep in registers
constexpr int kCStride = 128;
constexpr uint32_t kIdMask = 0x1fffffffu;
constexpr int kInReg8 = 16;          // entries of a row held in registers

constexpr int kLdsBlock = SGDNET_LDS_BLOCK;
constexpr int kDenseBlock = 256;
constexpr int kDenseVsBlock = 1024;             // dense K == 1 shards: 16 wavefronts share one LDS copy of the accumulator
constexpr int kTileF = 64;

// the slab sweeps (batched_sweep.hip, batched_shards.hip): a block owns kSlabElems (class, feature) entries
constexpr int kSlabElems = 32;
constexpr int kSlabGroups = kBlock / kSlabElems;

// ---- the fused epoch of the virtual shards (batched_shards.hip) ----
constexpr int kSyncLine = 32;                  // unsigned words per 128-B line: every polled word has a line of its own
constexpr int kSyncGo = 0, kSyncExit = 1, kSyncStart = 2, kSyncCnt1 = 3, kSyncCnt2 = kSyncCnt1 + 8,
              kSyncXcd = kSyncCnt2 + 8;
constexpr int kFusedMaxBps = 128;              // workgroups per shard
constexpr int kSyncLines = kSyncXcd + 8;         // (the slice counters col[i] of the merges have an array of their own: SagaDev::vcol)
constexpr int kSyncSticky = kSyncLines;        // abort code of any launch since the host last looked (never reset on the device)
constexpr int kSyncSeq = kSyncLines + 1;       // linked solvers: launches since they were linked (their slice counters run on)
constexpr int kFusedChunks = 3;                // 64-lane chunks of 16-byte pairs in a workgroup's feature slice
constexpr long long kFusedStartTicks = 2000000;      // 20 ms of the 100 MHz wall clock: the start barrier
constexpr long long kFusedWaitTicks = 200000000;     // 2 s: every later wait (never reached unless there is a bug)

// ---- the binned form (batched_binned.hip) ----
struct __attribute__((aligned(16))) BinEntry {
  uint32_t t;   // draw index inside the batch
  uint32_t j;   // feature
  double x;
};
static_assert(sizeof(BinEntry) == 16, "bin entries are 16 bytes");

constexpr int kBinBlock = SGDNET_BIN_BLOCK;   // gather+bin threads: one 16-lane group per draw in flight
constexpr int kBinDraws = kBinBlock / 2;      // draws per gather workgroup (8 passes)
constexpr int kBinEntCap = 7 * kBinBlock;     // LDS staging capacity (entries); beyond it entries go out one by one
constexpr int kBinW = SGDNET_BIN_W;           // reads of w requested together (8 or 16)
constexpr int kRangeBlock = SGDNET_RANGE_BLOCK;   // range sweep threads (78 VGPRs: 24 waves per CU)
constexpr size_t kRangeLdsBytes = 64 * 1024;

constexpr size_t kLdsPerCu = 160 * 1024;        // gfx950
constexpr size_t kLdsStaticReserve = 2 * 1024;  // static __shared__ of the LDS gather kernels
constexpr size_t kLdsTableMax = 80 * 1024;      // K x p accumulator the LDS forms stage (two workgroups per CU)
constexpr int kLdsCap = 96 * 1024;              // dynamic-LDS limit of the kernels that stage one such table
constexpr int kLdsAll = (int)(kLdsPerCu - kLdsStaticReserve);

// f(std::integral_constant<int, KW>{}) for the instance of class width kw <= 16 (KMAX template parameter)
template <typename F>
static int with_class_width(int kw, F&& f) {
  if (kw == 1) return f(std::integral_constant<int, 1>{});
  if (kw == 4) return f(std::integral_constant<int, 4>{});
  return f(std::integral_constant<int, 16>{});
}

// workgroups for `work` items at `per_block` each: at least one, at most `most`
static inline unsigned clamped_grid(int64_t work, int64_t per_block, int64_t most) {
  const int64_t grid = (work + per_block - 1) / per_block;
  return (unsigned)(grid < 1 ? 1 : grid > most ? most : grid);
}

// One kernel launch.  lds_cap > 0: the kernel's dynamic-LDS limit is raised to it first (once per device and kernel);
// ev0 / ev1 (optional): dispatch start / stop timestamps of exactly this kernel, used by the benchmark's per-kernel timing.
template <typename K, typename... A>
static int launch_kernel(K kernel, dim3 grid, dim3 block, size_t lds, int lds_cap, hipStream_t st, hipEvent_t ev0,
                         hipEvent_t ev1, const A&... args) {
  if (lds_cap > 0) {
    const int rc = allow_dynamic_lds(kernel, lds_cap);
    if (rc) return rc;
  }
  hipExtLaunchKernelGGL(kernel, grid, block, lds, st, ev0, ev1, 0, args...);
  SGD_HIP_TRY(hipGetLastError());
  return SGDNET_OK;
}

// the gather kernels of the LDS and dense forms share one signature: a launcher chooses among them by value
typedef void (*GatherKernel)(SagaDev, const LamParams*, int64_t, int, int, int);

// The per-family launchers the dispatching ones call.  (Hidden: the library exports what it exported as one file.)
#pragma GCC visibility push(hidden)
// batched_dense.hip
int launch_dense_gather(const SagaDev& d, const BatchPlan& g, LamParams* lam, int64_t t0_in_epoch, int m,
                        int batch_id_offset, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1);
int launch_dense_vs_gather(const SagaDev& d, const BatchPlan& g, LamParams* lam, int64_t t0_in_epoch, int m,
                           hipStream_t st, hipEvent_t ev0, hipEvent_t ev1, int batch_index);
int launch_dense_cl_sweep(const SagaDev& d, LamParams* lam, int tail, int n_parts, int batch_id_offset, hipStream_t st,
                          hipEvent_t ev0, hipEvent_t ev1);
// batched_binned.hip
int launch_binned_gather(const SagaDev& d, const BatchPlan& g, LamParams* lam, int64_t t0_in_epoch, int m,
                         int batch_id_offset, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1);
int launch_binned_sweep(const SagaDev& d, const BatchPlan& g, LamParams* lam, int penalty, int tail, int n_parts,
                        int batch_id_offset, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1);
#pragma GCC visibility pop

}  // namespace sgdnet
