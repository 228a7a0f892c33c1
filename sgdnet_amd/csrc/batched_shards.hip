// Batched SAGA, virtual shards: V locally normalised replicas of the state over V sample ranges.  The sweep of all
// replicas, their c . w, broadcast and merge kernels, and the fused epoch -- the whole epoch of all shards in one launch.
// (The shards' gather launches are those of the LDS and dense forms: launch_vs_gather, saga_batched.hip.)
#include "batched_k1.hpp"
#include "r_rng_bodies.hpp"

namespace sgdnet {

// --------------------------------------------------------------------------
// Virtual shards (K == 1): sweep of all V replicas in one launch.  Block b serves shard
// b / nfb and the 32 features (b % nfb) * 32 ...; it sums that shard's v_bps slabs in a fixed
// order, updates the shard's replica of (w, g_sum) with the shard's own normalisation, and the
// first block of every shard updates the shard's intercept pair.
// --------------------------------------------------------------------------
template <int KMAX>
__global__ __launch_bounds__(kBlock) void saga_vs_sweep_kernel(SagaDev d, LamParams* lamp, int tail, int nfb) {
  __shared__ double part[kSlabGroups][kSlabElems];
  __shared__ double red[kBlock / 64];
  __shared__ double sh_d0[KMAX];
  const SweepParams q = load_sweep_params(d, lamp, tail, SweepOverride{0.0, 0.0, 0.0});
  const int K = KMAX == 1 ? 1 : d.K;
  const int F = kSlabElems / K;              // features per block (K <= 16)
  const int E = F * K;
  const int v = (int)blockIdx.x / nfb, fb = (int)blockIdx.x - v * nfb;
  const int64_t KP = (int64_t)K * d.p;
  const double n_d = d.v_size[v];
  const int e = threadIdx.x % kSlabElems, g = threadIdx.x / kSlabElems;
  const int64_t elem = (int64_t)fb * E + e;
  // the updating threads' own coefficients and gradient averages: requested with the slabs, not behind them
  const int64_t j_own = (int64_t)fb * F + threadIdx.x;
  const bool updates = (int)threadIdx.x < F && j_own < d.p;
  double w_old[KMAX], g_old[KMAX], c_own = 0.0;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    w_old[k] = g_old[k] = 0.0;
    if (updates && k < K) {
      w_old[k] = d.vw[(int64_t)v * KP + j_own * K + k];
      g_old[k] = d.vG[(int64_t)v * KP + j_own * K + k];
    }
  }
  if (updates && d.standardize) c_own = d.c[j_own];
  double acc = 0.0;
  if (e < E && elem < KP) {
    const double* sp = d.slab + (int64_t)v * d.v_bps * KP + elem;
    int bidx = g;
    for (; bidx + 3 * kSlabGroups < d.v_bps; bidx += 4 * kSlabGroups) {   // 4 loads in flight
      const double a0 = sp[(int64_t)bidx * KP], a1 = sp[(int64_t)(bidx + kSlabGroups) * KP];
      const double a2 = sp[(int64_t)(bidx + 2 * kSlabGroups) * KP];
      const double a3 = sp[(int64_t)(bidx + 3 * kSlabGroups) * KP];
      acc += (a0 + a1) + (a2 + a3);
    }
    for (; bidx < d.v_bps; bidx += kSlabGroups) acc += sp[(int64_t)bidx * KP];
  }
  part[g][e] = acc;
  const bool need_d0 = fb == 0 || d.standardize;  // the shard's intercept accumulator = sum of gc, per class
  if (need_d0) {
    for (int k = 0; k < K; ++k) {
      double a = 0.0;
      for (int i = threadIdx.x; i < d.v_bps; i += kBlock) a += d.vd0[(int64_t)(v * d.v_bps + i) * K + k];
      a = wave_sum(a);
      if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
      __syncthreads();
      if (threadIdx.x == 0) {
        double t = 0.0;
        for (int wv = 0; wv < kBlock / 64; ++wv) t += red[wv];
        sh_d0[k] = t;
      }
      __syncthreads();
    }
  } else {
    __syncthreads();
  }
  if (updates) {
    double dj[KMAX], val[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      dj[k] = 0.0;
      if (k < K) {
        const int ee = (int)threadIdx.x * K + k;
        double t = 0.0;
        for (int gg = 0; gg < kSlabGroups; ++gg) t += part[gg][ee];
        dj[k] = t - (d.standardize ? c_own * sh_d0[k] : 0.0);   // implicit centring: D_j -= c_j * sum(gc)
      }
    }
    const double gls = q.gamma * q.ls_m;
    double nrm = 0.0;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      val[k] = k < K ? q.r_m * w_old[k] - gls * g_old[k] - q.gamma * dj[k] : 0.0;
      nrm += val[k] * val[k];
    }
    const double tau = q.beta * q.gamma * q.ls_m;
    const double factor = q.penalty == SGDNET_GROUPLASSO ? tau / sqrt(nrm) : 0.0;   // penalties.h:61-79
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      if (k < K) {
        double out = val[k];
        if (q.penalty == SGDNET_ELASTICNET) out = soft_threshold(out, tau);
        else if (q.penalty == SGDNET_GROUPLASSO) out = factor < 1.0 ? out * (1.0 - factor) : 0.0;
        d.vw[(int64_t)v * KP + j_own * K + k] = out;
        if (dj[k] != 0.0 || q.penalty == SGDNET_GROUPLASSO)
          d.vG[(int64_t)v * KP + j_own * K + k] = g_old[k] + dj[k] / n_d;
      }
    }
  }
  if (fb == 0 && (int)threadIdx.x < K && d.fit_intercept) {   // saga-sparse.h:300-304, batched form
    const int k = threadIdx.x;
    const double dk = sh_d0[k] / n_d;
    const double gbk = d.vgb[v * K + k] + dk;
    d.vgb[v * K + k] = gbk;
    d.vb[v * K + k] -= q.gamma * (gbk * (d.xd ? 1.0 : 0.01) * q.m_d + dk);
  }
}

// c . w of every replica and class (implicit centring)
__global__ __launch_bounds__(kBlock) void saga_vs_cw_kernel(SagaDev d) {
  __shared__ double red[kBlock / 64];
  const int K = d.K;
  const int v = (int)blockIdx.x / K, k = (int)blockIdx.x - v * K;
  const double* wv = d.vw + (int64_t)v * K * d.p + k;
  double a = 0.0;
  for (int64_t j = threadIdx.x; j < d.p; j += kBlock) a += d.c[j] * wv[j * K];
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int wvi = 0; wvi < kBlock / 64; ++wvi) t += red[wvi];
    d.vcw[blockIdx.x] = t;
  }
}

// replicated state, flattened: [g_sum (K p) | w (K p) | g_sum_intercept (K) | intercept (K)]
__device__ __forceinline__ double* vs_slot(const SagaDev& d, int v, int64_t i, int64_t KP, int K) {
  if (i < KP) return d.vG + (int64_t)v * KP + i;
  if (i < 2 * KP) return d.vw + (int64_t)v * KP + (i - KP);
  if (i < 2 * KP + K) return d.vgb + (int64_t)v * K + (i - 2 * KP);
  return d.vb + (int64_t)v * K + (i - 2 * KP - K);
}
__device__ __forceinline__ double* vs_own_slot(const SagaDev& d, int64_t i, int64_t KP, int K) {
  if (i < KP) return d.G + i;
  if (i < 2 * KP) return d.w + (i - KP);
  if (i < 2 * KP + K) return d.gb + (i - 2 * KP);
  return d.b + (i - 2 * KP - K);
}

// every replica (and the snapshot) <- the solver's current (w, g_sum, b, g_sum_b)
__global__ __launch_bounds__(kBlock) void saga_vs_broadcast_kernel(SagaDev d) {
  const int K = d.K;
  const int64_t KP = (int64_t)K * d.p, len = 2 * KP + 2 * K;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < len; i += (int64_t)gridDim.x * kBlock) {
    const double val = *vs_own_slot(d, i, KP, K);
    d.vref[i] = val;
    for (int v = 0; v < d.V; ++v) *vs_slot(d, v, i, KP, K) = val;
  }
}

// periodic average: every replica (and the snapshot) <- snapshot + sum_v (size_v / n) (replica_v - snapshot);
// final_merge also stores the result as the solver's state
// epoch_end != nullptr (the epoch's last merge): also the epoch's bookkeeping (saga_epoch_end_kernel), one launch less
__global__ __launch_bounds__(kBlock) void saga_vs_merge_kernel(SagaDev d, int final_merge, LamParams* epoch_end,
                                                               int batches) {
  if (epoch_end && blockIdx.x == 0 && threadIdx.x == 0) end_epoch(epoch_end, batches);
  const int K = d.K;
  const int64_t KP = (int64_t)K * d.p, len = 2 * KP + 2 * K;
  double tot_size = 0.0;
  for (int v = 0; v < d.V; ++v) tot_size += d.v_size[v];
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < len; i += (int64_t)gridDim.x * kBlock) {
    const double ref = d.vref[i];
    double val = ref;
    for (int v = 0; v < d.V; ++v) val += (d.v_size[v] / tot_size) * (*vs_slot(d, v, i, KP, K) - ref);
    d.vref[i] = val;
    for (int v = 0; v < d.V; ++v) *vs_slot(d, v, i, KP, K) = val;
    if (final_merge) *vs_own_slot(d, i, KP, K) = val;
  }
}

// --------------------------------------------------------------------------
// Fused epoch of the virtual shards (round 4): ONE launch per epoch instead of
// broadcast + 10 x (gather, sweep) + 5 merges.  Sparse x, one response, compact records.
//
// Between two merges the V shards are independent chains gather -> sweep -> gather ...
// (src/saga-sparse.h:258-337 in batches, per replica), so nothing but a merge needs the whole
// grid: the S workgroups of a shard synchronise among themselves (two counters per shard), and a
// merge needs only the V workgroups that own the same feature slice (one counter per slice).  The
// shards therefore drift apart in time: while one shard's workgroups publish slabs, wait, sweep
// and restage w -- all latency -- the other shards' draw loops keep the memory system busy.  With
// one launch per batch every workgroup of the chip went through those phases at the same moment
// (26 % of a C4 epoch was outside the draw loops: VERDICT round 3).
//
// Round r of workgroup (v, i) -- shard v, slice i of S:
//   stage    W (LDS) <- replica w_v ; b0 <- b_v [- c.w_v]                  (round 0: the solver's own state)
//   draws    its share of the shard's batch against (W, b0): K1Compact, D_i in LDS   (saga-sparse.h:274-282, 306-335)
//   publish  D_i -> slab (v, i), sum of gc -> vd0 ; arrive cnt1[v] ; wait for all S
//   sweep    features [i F, (i+1) F): sum of the S slabs in a fixed order, w_j <- r^m w_j - gamma LS_m G_j
//            - gamma D_j ; prox ; G_j += D_j / n_v (:316-325, 340-348 batched; penalties.h); (i == 0) intercept (:300-304)
//   merge    (every `every` rounds and at the end) slice -> pub[parity][v] ; arrive col[i] ; wait for all V ;
//            slice <- ref + sum_u (n_u / n) (pub_u - ref), the same expression in all V workgroups
//   arrive cnt2[v] ; wait for all S (next round's staging reads every slice of w_v)
//
// Visibility follows the write-through form of the CDNA4 guide (inter-workgroup hand-off, form R1): EVERY byte
// another workgroup reads is stored with sc1 (buffer_store ... sc1 / agent-scope atomic store), every storing wave
// drains vmcnt before the workgroup's barrier, ONE lane then adds to the counter (agent-scope atomic), ONE lane polls
// it with sc1 loads, the other waves wait at a workgroup barrier, and EVERY load of handed-off bytes is an sc1 load
// (no L1 hit on a stale line).  Nothing depends on which XCD a workgroup runs on.
//
// Residency: the workgroups spin on each other, so all of them must be resident at once (one per CU: the LDS
// tables fill it).  The kernel does not assume that: it opens with a start barrier that ONE arbiter word decides
// (compare-and-swap 0 -> 1 "go" by workgroup 0 once everybody has arrived, 0 -> 2 "abort" by whoever waited too
// long); before that decision nothing is modified, so an aborted launch (a GPU shared with another process, fewer
// CUs than the grid) leaves the solver's state as it was, LamParams::fused_abort = 1 tells the host, and the epoch is
// run again as separate launches.  Every later wait is bounded too (fused_abort = 2: a bug, the epoch is void).
// The last workgroup to leave zeroes the counters for the next launch.
// --------------------------------------------------------------------------

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
typedef double f64x2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ __amdgpu_buffer_rsrc_t fused_rsrc(const void* base, int64_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}
// 16-byte write-through store / L1-bypassing load (aux 16 = sc1)
__device__ __forceinline__ void st2_sc1(f64x2_t x, __amdgpu_buffer_rsrc_t rs, uint32_t byte_off) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, x), rs, (int)byte_off, 0, 16);
}
__device__ __forceinline__ f64x2_t ld2_sc1(__amdgpu_buffer_rsrc_t rs, uint32_t byte_off) {
  return __builtin_bit_cast(f64x2_t, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)byte_off, 0, 16));
}
// intra-shard hand-offs.  local: every workgroup of the shard runs on ONE XCD (verified at the start barrier from
// XCC_ID), whose L2 is the coherence point of its CUs: a plain store lands there and stays, and the consumers'
// L1-bypassing (sc1) loads are served from it -- nothing crosses the fabric.  Otherwise the write-through forms.
__device__ __forceinline__ void st2_shard(f64x2_t x, __amdgpu_buffer_rsrc_t rs, uint32_t byte_off, bool local) {
  if (local)
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, x), rs, (int)byte_off, 0, 0);
  else
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, x), rs, (int)byte_off, 0, 16);
}
__device__ __forceinline__ void st_shard(double* q, double x, bool local) {
  if (local)
    *q = x;
  else
    __hip_atomic_store(q, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_sc1(double* q, double x) {
  __hip_atomic_store(q, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld_sc1(const double* q) {
  return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// across GPUs (fine-grained memory of a peer or of this device that peers write): system scope
__device__ __forceinline__ void st_sys(double* q, double x) {
  __hip_atomic_store(q, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ double ld_sys(const double* q) {
  return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ unsigned sync_load(unsigned* sync, int word) {
  return __hip_atomic_load(sync + word * kSyncLine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// every wave of the workgroup has drained its stores; ONE lane signals
__device__ __forceinline__ void fused_arrive(unsigned* sync, int word) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0)
    __hip_atomic_fetch_add(sync + word * kSyncLine, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one lane: counter >= target, or give up (returns false; *fail set on a timeout of this lane's own)
// (system: the counter receives remote adds of linked solvers on other GPUs)
// ctr: the array the counter lives in (vsync, or vcol for the merges' slice counters); sync: vsync (go / abort words)
__device__ __forceinline__ bool fused_poll(unsigned* ctr, int word, unsigned target, LamParams* lamp, bool system = false,
                                           unsigned* sync = nullptr) {
  if (!sync) sync = ctr;
  const long long t0 = wall_clock64();
  for (unsigned spins = 1;; ++spins) {
    const unsigned now = system ? __hip_atomic_load(ctr + word * kSyncLine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)
                                : sync_load(ctr, word);
    if (now >= target) return true;
    __builtin_amdgcn_s_sleep(4);
    if ((spins & 63u) == 0) {
      if (sync_load(sync, kSyncGo) != 1u) return false;          // somebody else gave up
      if (wall_clock64() - t0 > kFusedWaitTicks) {
        __hip_atomic_store(sync + kSyncGo * kSyncLine, 3u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&lamp->fused_abort, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(sync + kSyncSticky * kSyncLine, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return false;
      }
    }
  }
}

// The start barrier (one lane per workgroup).  Returns true when the arbiter word says "go".
__device__ __forceinline__ bool fused_start(unsigned* sync, LamParams* lamp, unsigned grid) {
  unsigned* go = sync + kSyncGo * kSyncLine;
  const long long t0 = wall_clock64();
  if (blockIdx.x == 0) {
    unsigned expect = 0u;
    for (;;) {
      if (sync_load(sync, kSyncStart) >= grid) {
        __hip_atomic_compare_exchange_strong(go, &expect, 1u, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
      if (sync_load(sync, kSyncGo) != 0u) break;
      if (wall_clock64() - t0 > kFusedStartTicks) {
        __hip_atomic_compare_exchange_strong(go, &expect, 2u, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
      __builtin_amdgcn_s_sleep(4);
    }
  } else {
    for (;;) {
      if (sync_load(sync, kSyncGo) != 0u) break;
      if (wall_clock64() - t0 > 2 * kFusedStartTicks) {     // workgroup 0 itself is not running
        unsigned expect = 0u;
        __hip_atomic_compare_exchange_strong(go, &expect, 2u, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
      __builtin_amdgcn_s_sleep(4);
    }
  }
  const unsigned decision = sync_load(sync, kSyncGo);
  if (decision != 1u && decision != 3u) {
    __hip_atomic_store(&lamp->fused_abort, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(sync + kSyncSticky * kSyncLine, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  return decision == 1u;
}

// deterministic sum over the workgroup (every thread gets it); two barriers
__device__ __forceinline__ double fused_block_sum(double a, double* red) {
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int wv = 0; wv < kLdsBlock / 64; ++wv) t += red[wv];
  __syncthreads();
  return t;
}

// every workgroup leaves through here: the last one out resets the counters for the next launch (and moves the
// generators on when this launch produced a generation of the sample order)
__device__ __forceinline__ void fused_leave(const SagaDev& d, LamParams* lamp, int nb, bool epoch_done) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x < 64) {                       // wavefront 0: lane 0 signs out, every lane has a share of the reset
    unsigned* sync = d.vsync;
    unsigned prev = 0u;
    if (threadIdx.x == 0) {
      if (epoch_done && blockIdx.x == 0) {
        end_epoch(lamp, nb);
        // linked solvers: one more launch whose merges the slice counters have counted (this workgroup says so, not
        // the last one out: that may be a generators' workgroup, which knows nothing of the epoch)
        if (d.n_peers > 1) __hip_atomic_fetch_add(sync + kSyncSeq * kSyncLine, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      prev = __hip_atomic_fetch_add(sync + kSyncExit * kSyncLine, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    prev = (unsigned)__shfl((int)prev, 0);
    if (prev + 1u == gridDim.x) {
      // one lane per word: the stores of a pass leave together instead of one behind the other
      // (linked solvers: the other ranks add to this rank's slice counters whenever THEY get there -- those run on
      //  from launch to launch, with the launch count as their base)
      const int lane = (int)threadIdx.x;
      for (int wd = lane; wd < kSyncLines; wd += 64)
        __hip_atomic_store(sync + wd * kSyncLine, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (!(d.n_peers > 1))
        for (int wd = lane; wd < kFusedMaxBps; wd += 64)
          __hip_atomic_store(d.vcol + wd * kSyncLine, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (lane == 0 && d.rngdev && lamp->rng_generate) d.rngdev->gen += 1u;
    }
  }
}

// kPeers: the instantiation for linked solvers (the merge reaches over the ranks).  A template parameter, not a run-time
// branch: the draw loop has no register to spare, and the extra live values of the linked merge pushed three of its
// values into scratch (+20 % per epoch on ONE GPU, measured) -- the unlinked instantiation does not carry them.
template <bool kPeers>
__global__ __launch_bounds__(kLdsBlock) void saga_vs_epoch_kernel(SagaDev d, LamParams* lamp, int nb, int every) {
  extern __shared__ __attribute__((aligned(16))) double Dl[];
  __shared__ int ticket_counter;
  __shared__ int sh_ok;
  __shared__ double sh_red[kLdsBlock / 64];
  __shared__ double sh_val[4];                  // [0] b0 of the round, [1] sum of gc of the shard's batch, [2] b as the epoch starts
  const int tid = threadIdx.x;
  const int64_t p = d.p;                        // K == 1, p even
  const int64_t P2 = p >> 1;
  const int S = d.v_bps, V = d.V;
  if ((int)blockIdx.x >= V * S) {
    // ---- the generators' workgroups: the NEXT epoch's raw words, then the generators' start states one epoch on ----
    // (r_rng_bodies.hpp; nothing here waits for the epoch's workgroups, nor they for this)
    if (d.rngdev && lamp->rng_generate) {
      const RngDev* R = d.rngdev;
      const unsigned gen = R->gen;
      uint32_t* lds = reinterpret_cast<uint32_t*>(Dl);
      const int rb = (int)blockIdx.x - V * S, nrb = (int)gridDim.x - V * S;
      mt_state_body(rb, nrb, reinterpret_cast<uint32_t(*)[2][kMtN + 1]>(lds), R->state[gen & 1u], R->ends,
                    R->stream + (int64_t)(gen & 1u) * R->n, R->n, R->seg, R->gens);
      __syncthreads();
      mt_jump_body(rb, nrb, lds, R->state[gen & 1u], R->state[(gen + 1u) & 1u], R->poly, R->gens);
    }
    fused_leave(d, lamp, nb, false);
    return;
  }
  // workgroups are dealt round-robin over the XCDs: shard = index modulo V puts a shard's workgroups on one XCD when
  // V == 8 (speed only; what the hardware really did is checked at the start barrier)
  const int v = (int)blockIdx.x % V, wi = (int)blockIdx.x / V;
  const int F = 2 * (int)((p + 2 * S - 1) / (2 * S));            // features of a workgroup's slice (even)
  const int j0 = wi * F;
  const int jn = p - j0 < F ? (p - j0 > 0 ? (int)(p - j0) : 0) : F;
  double* Wl = Dl + p;
  f64x2_t* D2 = reinterpret_cast<f64x2_t*>(Dl);
  f64x2_t* W2 = reinterpret_cast<f64x2_t*>(Wl);
  // per-lambda parameters: read once (the epoch's bookkeeping rewrites LamParams at the end)
  const int penalty = lamp->penalty;
  // (the round's scalars are kept in LDS and read where they are used: as kernel-long register values they -- with the
  //  other uniform values of this kernel -- overflowed the scalar registers into vector registers the draw loop needs)
  __shared__ double sh_par[10];                 // gamma, beta, r_full, ls_full, r_tail, ls_tail, n_v, lo_v, total samples
  if (tid == 0) {
    sh_par[0] = lamp->gamma;
    sh_par[1] = lamp->beta;
    sh_par[2] = lamp->r_full;
    sh_par[3] = lamp->ls_full;
    sh_par[4] = lamp->r_tail;
    sh_par[5] = lamp->ls_tail;
    // the eight sizes are read together (constant indices: V <= 8 is the array's length), summed in the shards' order
    const int vv = (int)blockIdx.x % d.V;
    double tot = 0.0, lo = 0.0, own = 0.0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const double x = d.v_size[u];
      if (u < d.V) tot += x;
      if (u < vv) lo += x;
      if (u == vv) own = x;
    }
    sh_par[6] = own;
    sh_par[7] = lo;
    sh_par[8] = tot;
  }
  const int64_t m_full = lamp->m_full;
  const int64_t sbase = lamp->stream_base;
  const bool raw_words = lamp->stream_raw != 0;   // the stream holds the generators' raw words: a word becomes a draw where it is read (K1CompactT)
  const int64_t dps = d.v_dps;
  const bool std_x = d.standardize != 0;
  const int64_t L = 2 * p + 2;                  // [g_sum | w | g_sum_intercept | intercept]
  double* vwv = d.vw + (int64_t)v * p;
  double* vGv = d.vG + (int64_t)v * p;
  double* refv = d.vx + (int64_t)v * L;
  double* cwp = d.vx + (int64_t)V * L;          // c . w of every workgroup's slice: V x kFusedMaxBps
  unsigned* sync = d.vsync;
  const __amdgpu_buffer_rsrc_t rs_slab = fused_rsrc(d.slab, (int64_t)V * S * p * 8);
  const __amdgpu_buffer_rsrc_t rs_w = fused_rsrc(vwv, p * 8);
  // shard v's region of the sample order: draws, or the generators' raw words (raw_words); never written here
  const uint32_t* const stream_v = d.stream + sbase + (int64_t)v * dps;
  typedef K1CompactT<true> K1Epoch;
  const double* const draw_par = sh_par + 6;    // (n_v, lo_v)

#ifdef SGDNET_PHASE_TIMING
  // thread 0's time per phase, summed over the rounds: dbg[workgroup * 16 + phase]; slots 14 / 15: first and last stamp
  unsigned long long ph_t = 0;
  if (d.dbg && tid == 0) d.dbg[(size_t)blockIdx.x * 16 + 14] = ph_t = phase_stamp();
#define FPH(slot)                                                 \
  do {                                                            \
    if (d.dbg && tid == 0) {                                      \
      const unsigned long long now = phase_stamp();               \
      d.dbg[(size_t)blockIdx.x * 16 + (slot)] += now - ph_t;      \
      d.dbg[(size_t)blockIdx.x * 16 + 15] = ph_t = now;           \
    }                                                             \
  } while (0)
#else
#define FPH(slot) ((void)0)
#endif
  // ---- start barrier: before "go" nothing is modified in global memory ------------------------------------
  // The workgroup arrives first.  While the others arrive, round 0's cold reads are on their way: the first sample
  // words, their cmeta bits, b and the coefficients for LDS.  All of them are inputs that the launch before this one
  // completed; loads and LDS contents commit nothing, so a launch that gives up still leaves global memory as it was.
  if (tid == 0) {
    // which XCD runs this workgroup: the shard's workgroups OR their bits together before they arrive
    const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 15u;        // HW_REG_XCC_ID
    __hip_atomic_fetch_or(sync + (kSyncXcd + v) * kSyncLine, 1u << xcc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_fetch_add(sync + kSyncStart * kSyncLine, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  constexpr int kStage = 8;                     // one round of loads for up to 16 384 coefficients
  uint32_t s_first = 0u, s_second = 0u;
  {
    K1Epoch nx;
    nx.begin(d, stream_v, (int)(dps < m_full ? dps : m_full), wi, S, &ticket_counter);
    nx.raw = raw_words;
    nx.par = draw_par;
    f64x2_t t[kStage];
#pragma unroll
    for (int q = 0; q < kStage; ++q) {
      const int64_t i = tid + (int64_t)q * kLdsBlock;
      t[q] = f64x2_t{0.0, 0.0};
      if (i < P2) t[q] = reinterpret_cast<const f64x2_t*>(d.w)[i];
    }
    if (tid == 64) sh_val[2] = d.b[0];
    __syncthreads();                            // sh_par: a raw word becomes a sample id with (n_v, lo_v)
    nx.tag_first();
    s_first = nx.s_cur;                         // round 0: tagged already
    s_second = nx.s_nxt;
    if (tid == 0) {
      sh_ok = fused_start(sync, lamp, (unsigned)(V * S)) ? 1 : 0;
      if (sh_ok) {
        const unsigned mask = sync_load(sync, kSyncXcd + v);
        sh_ok = (mask & (mask - 1u)) == 0u ? 3 : 1;        // bit 1: the whole shard on one XCD
      }
    }
#pragma unroll
    for (int q = 0; q < kStage; ++q) {
      const int64_t i = tid + (int64_t)q * kLdsBlock;
      if (i < P2) W2[i] = t[q];
    }
    for (int64_t i = tid + (int64_t)kStage * kLdsBlock; i < P2; i += kLdsBlock)   // (no shape of today gets here)
      W2[i] = reinterpret_cast<const f64x2_t*>(d.w)[i];
  }
  for (int64_t i = tid; i < P2; i += kLdsBlock) D2[i] = f64x2_t{0.0, 0.0};
  __syncthreads();
#ifdef SGDNET_PHASE_TIMING
  // slots 8 / 9 / 10: "go" seen -> round 0 enters its draw loop; last round's stores issued -> the workgroup is out;
  // kernel entry -> "go" seen
  unsigned long long ph_go = 0;
  if (d.dbg && tid == 0) {
    ph_go = phase_stamp();
    d.dbg[(size_t)blockIdx.x * 16 + 10] = ph_go - ph_t;
  }
#endif
  bool done = false;
  bool alive = sh_ok != 0;
  unsigned col_base = 0u;                       // linked solvers: merges of the launches before this one
  if (kPeers) {
    int merges = 0;
    for (int r = 0; r < nb; ++r) merges += (r + 1 == nb || (r + 1) % every == 0) ? 1 : 0;
    col_base = sync_load(sync, kSyncSeq) * (unsigned)merges;
  }
  const bool local = (sh_ok & 2) != 0 && d.vs_xcd_local != 0;
  int mi = 0;                                   // merges so far
  // the sample ids of a round's first two passes are requested a phase ahead (round 0's: before the start barrier);
  // only they are carried over (the rest of K1Compact is lane geometry, set up again at the top of the round: fewer
  // registers live across the phases)
  for (int r = 0; alive && r < nb; ++r) {
    const int64_t t0 = (int64_t)r * m_full;
    const int m = (int)(dps - t0 < m_full ? dps - t0 : m_full);
    const bool tail = m != m_full;
    const bool last = r + 1 == nb;
    const bool merge_due = last || (r + 1) % every == 0;

    // ---- stage: long-row bits of the first draws (their ids were requested a phase ago), w, intercept --------
    if (tid == 0) ticket_counter = K1Epoch::static_tickets();
    K1Epoch cg;
    cg.init(d, stream_v + t0, m, wi, S, &ticket_counter);
    cg.raw = raw_words;
    cg.par = draw_par;
    cg.s_cur = s_first;
    cg.s_nxt = s_second;
    if (r > 0) cg.tag_first();
    int ts = threadIdx.x;                       // (opaque, as tq below)
    asm volatile("" : "+v"(ts));
    double cw = 0.0, bv = 0.0;                  // wave 0: requested in front of the staging loads (one round trip for all)
    if ((ts >> 6) == 0) {
      if (std_x && r > 0)
        for (int k = ts & 63; k < S; k += 64) cw += ld_sc1(cwp + v * kFusedMaxBps + k);
      bv = r == 0 ? sh_val[2] : ld_sc1(d.vb + v);
    }
    if (r > 0) {                                // (round 0's coefficients were staged before the start barrier)
      for (int64_t i0 = ts; i0 < P2; i0 += (int64_t)kLdsBlock * kStage) {
        f64x2_t t[kStage];
#pragma unroll
        for (int q = 0; q < kStage; ++q) {
          const int64_t i = i0 + (int64_t)q * kLdsBlock;
          t[q] = f64x2_t{0.0, 0.0};
          if (i < P2) t[q] = ld2_sc1(rs_w, (uint32_t)(i * 16));
        }
#pragma unroll
        for (int q = 0; q < kStage; ++q) {
          const int64_t i = i0 + (int64_t)q * kLdsBlock;
          if (i < P2) W2[i] = t[q];
        }
      }
    }
    if ((ts >> 6) == 0) {                       // b0 = b_v - c . w_v
      cw = wave_sum(cw);
      if ((ts & 63) == 0) sh_val[0] = bv - cw;
    }
    __syncthreads();
    if (r == 0 && std_x) {                      // c . w of the state the epoch starts from
      double a = 0.0;
      for (int64_t j = ts; j < p; j += kLdsBlock) a += d.c[j] * Wl[j];
      a = fused_block_sum(a, sh_red);
      if (ts == 0) sh_val[0] -= a;
      __syncthreads();
    }
    const double b0 = sh_val[0];
    FPH(0);
#ifdef SGDNET_PHASE_TIMING
    if (d.dbg && tid == 0 && r == 0) d.dbg[(size_t)blockIdx.x * 16 + 8] = ph_t - ph_go;
#endif

    // ---- draws ------------------------------------------------------------------------------
    const double gct = cg.run(d, b0, Wl, Dl);
    __syncthreads();
    FPH(1);
    // (an opaque copy of the thread id: nothing computed from it below can be hoisted out of the round and kept in
    //  registers across the draw loop, which has none to spare)
    int tq = threadIdx.x;
    asm volatile("" : "+v"(tq));
    const int lane = tq & 63, wave = tq >> 6;
    const int64_t t0n = t0 + m_full;
    const int mn = (int)(dps - t0n < m_full ? dps - t0n : m_full);

    // ---- publish the slab (write-through) and the sum of the gradient changes -----------------------
    {
      const uint32_t base = (uint32_t)(((int64_t)blockIdx.x * p) * 8);
      for (int64_t i = tq; i < P2; i += kLdsBlock) {
        st2_shard(D2[i], rs_slab, base + (uint32_t)(i * 16), local);
        D2[i] = f64x2_t{0.0, 0.0};
      }
      const double t = wave_sum(gct);
      if (lane == 0) sh_red[wave] = t;
      __syncthreads();
      if (tq == 0) {
        double tot = 0.0;
        for (int wv = 0; wv < kLdsBlock / 64; ++wv) tot += sh_red[wv];
        st_shard(d.vd0 + blockIdx.x, tot, local);
      }
    }
    fused_arrive(sync, kSyncCnt1 + v);
    FPH(2);
    // behind the arrival, while the rest of the shard finishes: this workgroup's own coefficients (nobody else
    // writes them).
    // A thread owns one PAIR (A, B) of the replicated state: (g_sum_j, w_j) of its feature j, or -- the first thread
    // past the slice in the shard's workgroup 0 -- (g_sum_intercept, intercept): sweep and merge treat both alike
    // (fewer values in flight than two code paths: the phases of this kernel compete with the draw loop for registers)
    const bool upd = tq < jn;
    const bool icpt = wi == 0 && tq == jn;
    const bool act = upd || icpt;
    const int64_t j = j0 + tq;
    const int64_t oa = upd ? j : 2 * p, ob = upd ? p + j : 2 * p + 1;      // offsets in [g_sum | w | g_sum_b | b]
    double* const rep_a = upd ? vGv + j : d.vgb + v;                        // the replica's pair
    double* const rep_b = upd ? vwv + j : d.vb + v;
    const double* const own_a = upd ? d.G + j : d.gb;                       // the solver's own state (the epoch's start)
    const double* const own_b = upd ? d.w + j : d.b;
    double a_old = 0.0, b_old = 0.0, c_own = 0.0, ra = 0.0, rb = 0.0;
    if (act) {
      a_old = r == 0 ? *own_a : ld_sc1(rep_a);
      b_old = r == 0 ? *own_b : ld_sc1(rep_b);
      if (std_x && upd) c_own = d.c[j];
      if (merge_due) {
        ra = mi == 0 ? *own_a : ld_sc1(refv + oa);
        rb = mi == 0 ? *own_b : ld_sc1(refv + ob);
      }
    }
    if (tq == 0) sh_ok = fused_poll(sync, kSyncCnt1 + v, (unsigned)S * (unsigned)(r + 1), lamp) ? 1 : 0;
    __syncthreads();
    if (!sh_ok) break;
    FPH(3);

    // ---- sweep of this workgroup's feature slice ------------------------------------------------
    {
      double gsum = 0.0;                        // requested in front of the slab loads
      if (wave == kLdsBlock / 64 - 1)
        for (int k = lane; k < S; k += 64) gsum += ld_sc1(d.vd0 + k * V + v);
      f64x2_t acc[kFusedChunks];
#pragma unroll
      for (int c = 0; c < kFusedChunks; ++c) acc[c] = f64x2_t{0.0, 0.0};
      for (int k = wave; k < S; k += 2 * (kLdsBlock / 64)) {
        const bool two = k + kLdsBlock / 64 < S;
        const uint32_t o0 = (uint32_t)((((int64_t)(k * V + v)) * p + j0) * 8);
        const uint32_t o1 = (uint32_t)((((int64_t)((k + kLdsBlock / 64) * V + v)) * p + j0) * 8);
        f64x2_t a0[kFusedChunks], a1[kFusedChunks];
#pragma unroll
        for (int c = 0; c < kFusedChunks; ++c) {
          const int pi = c * 64 + lane;
          a0[c] = a1[c] = f64x2_t{0.0, 0.0};
          if (2 * pi < jn) {
            a0[c] = ld2_sc1(rs_slab, o0 + (uint32_t)(pi * 16));
            if (two) a1[c] = ld2_sc1(rs_slab, o1 + (uint32_t)(pi * 16));
          }
        }
#pragma unroll
        for (int c = 0; c < kFusedChunks; ++c) {
          acc[c] += a0[c];
          acc[c] += a1[c];
        }
      }
#pragma unroll
      for (int c = 0; c < kFusedChunks; ++c) {
        const int pi = c * 64 + lane;
        if (2 * pi < F) reinterpret_cast<f64x2_t*>(Wl + (int64_t)wave * F)[pi] = acc[c];
      }
      if (wave == kLdsBlock / 64 - 1) {         // the shard's sum of gc (intercept accumulator; implicit centring)
        gsum = wave_sum(gsum);
        if (lane == 0) sh_val[1] = gsum;
      }
    }
    __syncthreads();
    double a_new = a_old, b_new = b_old;        // (g_sum, w) of the feature, or (g_sum_intercept, intercept)
    {
      const double d0 = sh_val[1];
      const double n_d = sh_par[6], gamma = sh_par[0];
      if (upd) {
        double dj = 0.0;
#pragma unroll
        for (int wv = 0; wv < kLdsBlock / 64; ++wv) dj += Wl[(int64_t)wv * F + tq];
        if (std_x) dj -= c_own * d0;            // implicit centring: D_j -= c_j * sum(gc)
        const double beta = sh_par[1];
        const double r_m = tail ? sh_par[4] : sh_par[2], ls_m = tail ? sh_par[5] : sh_par[3];
        const double val = r_m * b_old - (gamma * ls_m) * a_old - gamma * dj;
        const double tau = beta * gamma * ls_m;
        b_new = val;
        if (penalty == SGDNET_ELASTICNET) {
          b_new = soft_threshold(val, tau);
        } else if (penalty == SGDNET_GROUPLASSO) {          // penalties.h:61-79 with one response
          const double factor = tau / sqrt(val * val);
          b_new = factor < 1.0 ? val * (1.0 - factor) : 0.0;
        }
        a_new = (dj != 0.0 || penalty == SGDNET_GROUPLASSO) ? a_old + dj / n_d : a_old;
      } else if (icpt && d.fit_intercept) {     // saga-sparse.h:300-304 in batches
        const double dk = d0 / n_d;
        a_new = a_old + dk;
        b_new = b_old - gamma * (a_new * (d.xd ? 1.0 : 0.01) * (double)m + dk);
      }
    }
    FPH(4);
    if (merge_due) {
      // ---- periodic average of the replicas, slice by slice ------------------------------------------
      // Linked solvers (one per GPU of a node, SagaDev::peers): the average runs over the replicas of EVERY rank.
      // A workgroup publishes its slice in its own exchange buffer, adds to counter col[i] of every rank (remote
      // atomics over xGMI), waits for its own counter and reads the ranks' buffers with direct loads: the
      // "all-reduce" of this scheme is 2 (p / S) doubles per workgroup and shard, inside the epoch's one launch.
      // Those buffers and counters are fine-grained allocations, the accesses system-scope (sc0 sc1).
      const FusedPeers* PR = kPeers ? d.peers : nullptr;
      const int NP = kPeers ? d.n_peers : 1;
      double* pubv = d.vpub + (int64_t)((mi & 1) * V + v) * L;
      if (PR) {
        if (act) {
          st_sys(pubv + oa, a_new);
          st_sys(pubv + ob, b_new);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tq == 0)
          for (int q = 0; q < NP; ++q)
            __hip_atomic_fetch_add(PR->sync[q] + wi * kSyncLine, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      } else {
        if (act) {
          st_sc1(pubv + oa, a_new);
          st_sc1(pubv + ob, b_new);
        }
        fused_arrive(d.vcol, wi);
      }
      if (tq == 0)
        sh_ok = fused_poll(d.vcol, wi, (unsigned)(NP * V) * (col_base + (unsigned)(mi + 1)), lamp, PR != nullptr, sync) ? 1 : 0;
      __syncthreads();
      if (!sh_ok) break;
      double ma = ra, mb = rb;
      const double tot_all = PR ? PR->tot_size : sh_par[8];
      for (int q = 0; q < NP; ++q) {              // rank after rank, shard after shard: the same order everywhere
        const double* pub0 = (PR ? PR->pub[q] : d.vpub) + (int64_t)((mi & 1) * V) * L;
        double xa[8], xb[8];                      // every load of a rank's exchange first: one round trip
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          xa[u] = xb[u] = 0.0;
          if (u < V && act) {
            xa[u] = PR ? ld_sys(pub0 + (int64_t)u * L + oa) : ld_sc1(pub0 + (int64_t)u * L + oa);
            xb[u] = PR ? ld_sys(pub0 + (int64_t)u * L + ob) : ld_sc1(pub0 + (int64_t)u * L + ob);
          }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          if (u < V) {
            const double wt = (PR ? PR->vsize[q][u] : d.v_size[u]) / tot_all;
            ma += wt * (xa[u] - ra);
            mb += wt * (xb[u] - rb);
          }
        }
      }
      if (act) {
        a_new = ma;
        b_new = mb;
        // The reference copy is read at the NEXT merge of this launch; a later launch starts from the solver's own
        // state (mi == 0) and writes the copy before it reads it.  So the epoch's last merge skips it -- except shard
        // 0's, kept beside the own state it equals.
        if (!last || v == 0) {
          st_sc1(refv + oa, ma);
          st_sc1(refv + ob, mb);
        }
        if (last && v == 0) {                     // the solver's own state: what the epoch returns
          *const_cast<double*>(own_a) = ma;
          *const_cast<double*>(own_b) = mb;
        }
      }
      ++mi;
      FPH(5);
    }
    if (act) {
      st_shard(rep_a, a_new, local);
      st_shard(rep_b, b_new, local);
    }
    if (std_x && !last) {                       // c . w of the slice, for the next round's linear predictors (round 0 of
                                                // the next launch sums c . w itself: nothing reads the last round's)
      const double a = fused_block_sum(upd ? c_own * b_new : 0.0, sh_red);
      if (tq == 0) st_shard(cwp + v * kFusedMaxBps + wi, a, local);
    }
    if (last) {
      done = true;
      break;
    }
    fused_arrive(sync, kSyncCnt2 + v);
    FPH(6);
    // the next round's first sample ids (or raw words), requested before the wait
    {
      K1Epoch nx;
      nx.begin(d, stream_v + t0n, mn, wi, S, &ticket_counter);
      s_first = nx.s_cur;
      s_second = nx.s_nxt;
    }
    if (tq == 0) sh_ok = fused_poll(sync, kSyncCnt2 + v, (unsigned)S * (unsigned)(r + 1), lamp) ? 1 : 0;
    __syncthreads();
    if (!sh_ok) break;
    FPH(7);
  }

#ifdef SGDNET_PHASE_TIMING
  if (d.dbg && tid == 0) ph_t = phase_stamp();
#endif
  fused_leave(d, lamp, nb, done);
#ifdef SGDNET_PHASE_TIMING
  if (d.dbg && tid == 0) d.dbg[(size_t)blockIdx.x * 16 + 9] = phase_stamp() - ph_t;
#endif
}

// ------------------------------ launchers ---------------------------------
int launch_vs_broadcast(const SagaDev& d, hipStream_t st) {
  const int64_t len = 2 * (int64_t)d.K * d.p + 2 * d.K;
  return launch_kernel(saga_vs_broadcast_kernel, dim3(clamped_grid(len, kBlock, 1024)), dim3(kBlock), 0, 0, st, nullptr,
                       nullptr, d);
}

int launch_vs_cw(const SagaDev& d, hipStream_t st) {
  if (!d.standardize) return SGDNET_OK;
  return launch_kernel(saga_vs_cw_kernel, dim3(d.V * d.K), dim3(kBlock), 0, 0, st, nullptr, nullptr, d);
}

int launch_vs_merge(const SagaDev& d, int final_merge, hipStream_t st, LamParams* epoch_end, int batches) {
  const int64_t len = 2 * (int64_t)d.K * d.p + 2 * d.K;
  return launch_kernel(saga_vs_merge_kernel, dim3(clamped_grid(len, kBlock, 1024)), dim3(kBlock), 0, 0, st, nullptr,
                       nullptr, d, final_merge, epoch_end, batches);
}

int launch_vs_sweep(const SagaDev& d, const BatchPlan& g, LamParams* lam, int tail, hipStream_t st, hipEvent_t ev0,
                    hipEvent_t ev1) {
  const int F = kSlabElems / d.K;            // features per block
  const int nfb = (int)((d.p + F - 1) / F);
  return with_class_width(g.kw, [&](auto kw) {
    return launch_kernel(saga_vs_sweep_kernel<decltype(kw)::value>, dim3(nfb * d.V), dim3(kBlock), 0, 0, st, ev0, ev1, d,
                         lam, tail, nfb);
  });
}

int launch_vs_epoch(const SagaDev& d, const BatchPlan& g, LamParams* lam, int nb, int every, hipStream_t st,
                    hipEvent_t ev0, hipEvent_t ev1) {
  if (nb < 1 || every < 1) return SGDNET_EINVAL;
  const bool peers = d.n_peers > 1 && d.peers;
  return launch_kernel(peers ? saga_vs_epoch_kernel<true> : saga_vs_epoch_kernel<false>, dim3(g.grid), dim3(kLdsBlock),
                       g.lds_bytes, kLdsAll, st, ev0, ev1, d, lam, nb, every);
}

}  // namespace sgdnet
