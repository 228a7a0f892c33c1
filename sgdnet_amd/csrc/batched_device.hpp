// Batched SAGA, device helpers that more than one kernel family uses: group reductions and atomics, the d0 / c.w slot
// sets, the packed sample records and their one walker, the scatter, the phase stamps and the pieces of the sweeps.
#pragma once

#include "batched_geometry.hpp"
#include "device_math.hpp"

namespace sgdnet {

namespace {

// sum / maximum over a group of kGrp lanes: 8 (K == 1 forms), 16 (a draw's group, class-lane groups) or a whole wavefront
template <int kGrp>
__device__ __forceinline__ double grp_sum(double v) {
#pragma unroll
  for (int off = kGrp / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kGrp);
  return v;
}
template <int kGrp>
__device__ __forceinline__ double grp_max(double v) {
#pragma unroll
  for (int off = kGrp / 2; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, kGrp));
  return v;
}

__device__ __forceinline__ void atomic_add_f64(double* p, double v) {
  // no-return global_atomic_add_f64
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void atomic_max_bits(unsigned long long* p, double v) {
  // v >= 0: the IEEE bit pattern is monotone in v
  __hip_atomic_fetch_max(p, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
}

// Implicit centring of sparse x (standardize = TRUE; reference saga-sparse.h:127-128,
// 276-277 does it with dense O(p) work per iteration).  Against a snapshot of w it folds into
// two per-batch scalars per class: lp -= c.w and D_j -= c_j * sum_i gc_i.  c.w lives in two
// sets of 16 accumulation slots: the sweep of batch B adds its blocks' partial sums of
// c_j * w_new into set (B+1)&1 (zeroed by gather B), gather B+1 reads that set.
constexpr int kCwSlots = 16;

__device__ __forceinline__ double* d0_set(const SagaDev& d, int batch_id) {
  return d.d0_part + (size_t)(batch_id & 1) * kD0Slots * d.K;
}

__device__ __forceinline__ void d0_publish(const SagaDev& d, int batch_id, int k, double tot) {
  double* set = d0_set(d, batch_id);
  if (gridDim.x <= (unsigned)kD0Slots)
    set[(size_t)blockIdx.x * d.K + k] = tot;
  else if (tot != 0.0)
    __hip_atomic_fetch_add(set + (size_t)(blockIdx.x % kD0Slots) * d.K + k, tot, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}

// The epoch's bookkeeping on the device (captured epoch graphs replay without the host touching LamParams):
// the next epoch's draws follow this one's -- in the two-epoch buffer of the sample-order pipeline, in the other half.
__device__ __forceinline__ void end_epoch(LamParams* lamp, int batches) {
  int64_t sb = lamp->stream_base + lamp->draws_per_epoch;
  if (lamp->stream_wrap > 0 && sb >= lamp->stream_wrap) sb -= lamp->stream_wrap;
  lamp->stream_base = sb;
  lamp->batch_seq += batches;
}

__device__ __forceinline__ double cw_sum(const SagaDev& d, int batch_id, int k) {
  const double* set = d.cw + (size_t)(batch_id & 1) * kCwSlots * d.K;
  double t = 0.0;
#pragma unroll
  for (int i = 0; i < kCwSlots; ++i) t += set[i * d.K + k];
  return t;
}

__device__ __forceinline__ void cw_clear_next(const SagaDev& d, int batch_id) {
  if (blockIdx.x == 0 && (int)threadIdx.x < kCwSlots * d.K)
    d.cw[(size_t)((batch_id + 1) & 1) * kCwSlots * d.K + threadIdx.x] = 0.0;
}

}  // namespace

// --------------------------------------------------------------------------
// Packed sample records (built once per solver, solver.cpp: build_records).
// Random full 128-B lines stream at the HBM rate on MI355X (26 G random 256-B records/s,
// scripts/microbench/gather_rate.hip), partial lines waste it, and every dependent hop is a
// 1-2.5 us round trip, so a draw should touch as few lines as possible, whole, with no
// pointer hop:
//
//   record s at rec + s*stride (stride = 128-B multiple sized for the 90th
//   percentile row; requests are served in 128-B units):  [f64 y][i32 nnz][i32 ovf][i32 idx[cap]] pad8 [f64 val[cap]]
//   rows longer than cap continue in 256-B overflow records:
//                     [i32 next][i32 cnt][i32 idx[20]][f64 val[20]]
//
// At z = 10 a draw is one 256-B record = 2 requests (was: 2 row pointers + y + idx + val ~ 6).
// --------------------------------------------------------------------------
__device__ __forceinline__ double* m_slot(const SagaDev& d, int64_t s) {
  // gradient memory of sample s for the one-response sparse kernels: inside the compact record while the
  // solver keeps it there (solver.cpp: m_to_record / m_to_array), else the K x n array
  // (base and stride are kept by the host: a select between the two addresses in front of the atomic
  //  exchange sends this compiler's instcombine into a segmentation fault)
  return reinterpret_cast<double*>(d.m_base + (size_t)s * (size_t)d.m_stride);
}

constexpr int kOvfStride = 256;
constexpr int kOvfCap = 20;

// entries kFirst + lane, kFirst + lane + kStride, ... of the main record, then lane, lane + kStride, ... of every
// overflow record; (kStride == 1, lane == 0): every lane visits every entry (uniform addresses: broadcast loads)
template <int kFirst, int kStride, class F>
__device__ __forceinline__ void row_for_each(const SagaDev& d, const char* base, int nnz, int ovf, int lane, F f) {
  const int cap = d.rec_cap;
  const int cnt0 = nnz < cap ? nnz : cap;
  const int* ridx = reinterpret_cast<const int*>(base + 16);
  const double* rval = reinterpret_cast<const double*>(base + d.rec_val_off);
  for (int e = kFirst + lane; e < cnt0; e += kStride) f(ridx[e], rval[e]);
  int rem = nnz - cnt0;
  while (rem > 0) {
    const char* ob = d.ovf + (size_t)ovf * kOvfStride;
    const int next = reinterpret_cast<const int*>(ob)[0];
    const int c = reinterpret_cast<const int*>(ob)[1];
    const int* oi = reinterpret_cast<const int*>(ob + 8);
    const double* ov = reinterpret_cast<const double*>(ob + 8 + 4 * kOvfCap);
    for (int e = lane; e < c; e += kStride) f(oi[e], ov[e]);
    rem -= c;
    ovf = next;
  }
}

// kLds: the target is a workgroup-private LDS table (ds_add_f64), else global memory (global_atomic_add_f64)
template <bool kLds>
__device__ __forceinline__ void scatter_add(double* p, double v) {
  if (kLds)
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  else
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Intercept accumulator: one partial per block and class, summed by the sweep in a
// fixed order (thousands of same-address atomics would serialise at ~12 ns each).
template <int KMAX, int kThreads>
__device__ __forceinline__ void store_d0_partial(const SagaDev& d, int K, int batch_id,
                                                 const double (&gc)[KMAX]) {
  __shared__ double part[kThreads / 64][KMAX];
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    if (k < K) {
      const double tot = wave_sum(gc[k]);
      if ((threadIdx.x & 63) == 0) part[wave][k] = tot;
    }
  }
  __syncthreads();
  if (threadIdx.x < K) {
    double tot = 0.0;
#pragma unroll
    for (int wv = 0; wv < kThreads / 64; ++wv) tot += part[wv][threadIdx.x];
    d0_publish(d, batch_id, threadIdx.x, tot);
  }
}

#ifdef SGDNET_PHASE_TIMING
// development aid (never in the product build): shader-clock stamps after all outstanding
// memory operations of the wave have returned
__device__ __forceinline__ unsigned long long phase_stamp() {
  unsigned long long t;
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}
#define PHASE(slot)                                                                      \
  do {                                                                                    \
    if (d.dbg && threadIdx.x == 0) d.dbg[(size_t)blockIdx.x * 16 + (slot)] = phase_stamp(); \
  } while (0)
#define PHASE_FIRST(slot)                                                                 \
  do {                                                                                    \
    if (d.dbg && threadIdx.x == 0 && stamp) d.dbg[(size_t)blockIdx.x * 16 + (slot)] = phase_stamp(); \
  } while (0)
#else
#define PHASE(slot) ((void)0)
#define PHASE_FIRST(slot) ((void)0)
#endif

// --------------------------------------------------------------------------
// sweep: per feature (all K classes: GroupLasso needs the column norm)
//   w_j <- r^m w_j - gamma LS_m G_j - gamma D_j ; prox ; G_j += D_j / n
// --------------------------------------------------------------------------
struct SweepParams {
  int penalty;
  double gamma, beta, r_m, ls_m, m_d, n_d;
};

// Batch factors passed by value instead of read from LamParams (synchronous sharded mode: the
// draw count of a global batch varies by a few draws from round to round).  m <= 0: unused.
struct SweepOverride {
  double r_m, ls_m, m;
};

__device__ __forceinline__ SweepParams load_sweep_params(const SagaDev& d, const LamParams* lamp, int tail,
                                                         const SweepOverride& ov) {
  SweepParams q;
  q.penalty = lamp->penalty;
  q.gamma = lamp->gamma;
  q.beta = lamp->beta;
  q.r_m = tail ? lamp->r_tail : lamp->r_full;
  q.ls_m = tail ? lamp->ls_tail : lamp->ls_full;
  q.m_d = (double)(tail ? lamp->m_tail : lamp->m_full);
  if (ov.m > 0.0) {
    q.r_m = ov.r_m;
    q.ls_m = ov.ls_m;
    q.m_d = ov.m;
  }
  q.n_d = d.n_total;
  return q;
}

// dj: the K scatter sums of feature j (registers); wout receives the updated coefficients
__device__ __forceinline__ void sweep_feature(const SagaDev& d, const SweepParams& q, int64_t j,
                                              const double* dj, double* wout) {
  const int K = d.K;
  double* wj = d.w + j * K;
  double* gj = d.G + j * K;
  const double gls = q.gamma * q.ls_m;
  if (q.penalty == SGDNET_GROUPLASSO) {
    double nrm = 0.0;
    for (int k = 0; k < K; ++k) {
      const double v = q.r_m * wj[k] - gls * gj[k] - q.gamma * dj[k];
      wout[k] = v;
      nrm += v * v;
    }
    nrm = sqrt(nrm);
    const double factor = q.beta * q.gamma * q.ls_m / nrm;
    for (int k = 0; k < K; ++k) {
      wout[k] = factor < 1.0 ? wout[k] * (1.0 - factor) : 0.0;
      wj[k] = wout[k];
      gj[k] += dj[k] / q.n_d;
    }
  } else {
    const double tau = q.beta * q.gamma * q.ls_m;
    for (int k = 0; k < K; ++k) {
      const double dk = dj[k];
      double v = q.r_m * wj[k] - gls * gj[k] - q.gamma * dk;
      if (q.penalty == SGDNET_ELASTICNET) v = soft_threshold(v, tau);
      wj[k] = v;
      wout[k] = v;
      if (dk != 0.0) gj[k] += dk / q.n_d;
    }
  }
}

// d0[k] = sum of the gather kernel's per-block partials, in a fixed order, for every thread of
// the block (result in sh_d0).  Called by whole blocks.
template <int kThreads>
__device__ __forceinline__ void block_d0(const SagaDev& d, int n_parts, int batch_id, double* sh_d0) {
  __shared__ double red[kThreads / 64];
  const int K = d.K;
  for (int k = 0; k < K; ++k) {
    double acc = 0.0;
    const double* set = d0_set(d, batch_id);
    for (int i = threadIdx.x; i < n_parts; i += kThreads) acc += set[(int64_t)i * K + k];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      double tot = 0.0;
      for (int wv = 0; wv < kThreads / 64; ++wv) tot += red[wv];
      sh_d0[k] = tot;
    }
    __syncthreads();
  }
}

// intercept: gb += d0/n ; b -= gamma (0.01 m gb + d0/n)   (saga-sparse.h:300-304)
__device__ __forceinline__ void sweep_intercept(const SagaDev& d, const SweepParams& q, const double* sh_d0) {
  if ((int)threadIdx.x < d.K) {
    const int k = threadIdx.x;
    const double dk = sh_d0[k] / q.n_d;
    const double gbk = d.gb[k] + dk;
    d.gb[k] = gbk;
    // sparse x: the reference's intercept decay 0.01 (saga-sparse.h:300-304); dense x: none (saga-dense.h:170-173)
    d.b[k] -= q.gamma * (gbk * (d.xd ? 1.0 : 0.01) * q.m_d + dk);
  }
}

// adds this block's sum of c_j * w_new_kj into the next batch's c.w slots
template <int kThreads>
__device__ __forceinline__ void cw_accumulate(const SagaDev& d, int batch_id, const double* cwp) {
  __shared__ double red[kThreads / 64][64];
  const int K = d.K;
  for (int k = 0; k < K; ++k) {
    const double t = wave_sum(cwp[k]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = t;
  }
  __syncthreads();
  if ((int)threadIdx.x < K) {
    double tot = 0.0;
    for (int wv = 0; wv < kThreads / 64; ++wv) tot += red[wv][threadIdx.x];
    double* set = d.cw + (size_t)((batch_id + 1) & 1) * kCwSlots * K;
    if (tot != 0.0) atomic_add_f64(set + (blockIdx.x % kCwSlots) * K + threadIdx.x, tot);
  }
}

}  // namespace sgdnet
