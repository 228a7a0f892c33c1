// Batched ("B-stale") sparse SAGA kernels for gfx950: the throughput path.
//
// A batch is `m` consecutive draws of the sample stream evaluated against one
// snapshot of (w, intercept).  In unscaled coordinates (true w = wscale * w of
// the reference) the reference iteration src/saga-sparse.h:258-337 applied to
// the batch becomes, per feature j (DESIGN.md "Batched mode"):
//
//   gather : per draw i   lp = w . x_s + b ; g = Gradient(lp, y_s)            (:274, :279)
//                         gc = g - g_memory[s] ; g_memory[s] = g              (:281-282)
//                         D[:, j] += x_sj * gc   for j in nz(x_s)             (:306-313, :328-335)
//   sweep  : per feature  w_j = r^m w_j - gamma LS_m G_j - gamma D_j ; prox   (:316-325 + penalties.h)
//                         G_j += D_j / n ;  D_j = 0
//            intercept    gb += d0/n ; b -= gamma (0.01 m gb + d0/n)          (:300-304; dense x: m gb, saga-dense.h:170-173)
//
// with r = 1 - alpha*gamma and LS_m = sum_{k<m} r^k (= lag_scaling[m], :229-240).
// m == 1 is the reference iteration itself.  A sample drawn twice inside one
// batch sees the same snapshot, so its second draw has gc == 0: the first draw
// claims the sample (atomic exchange) and later ones contribute nothing.
//
// Memory behaviour: the gather kernel is the HBM-bound one -- per draw it pulls
// one stream entry, the sample's packed record (y, z indices, z values) and the
// gradient memory (algorithmic 16 + 12 z + 16 K bytes) at random
// sample positions; 16-lane groups own one draw so that a wavefront has 4
// independent gathers in flight and reduces x.w with intra-row shuffles.  w, D
// and G are K*p doubles (80 KB at 10k features) and stay L2 / Infinity-Cache
// resident.
//
// This unit holds the sparse gather forms -- global-atomic, LDS-privatised, class-lane -- with the packing of the
// compact records; the other kernel families of the batched iteration are batched_dense.hip, batched_sweep.hip,
// batched_shards.hip and batched_binned.hip, the rule that chooses between them is plan_batch (batched_plan.cpp).
#include "batched_k1.hpp"

namespace sgdnet {

// --------------------------------------------------------------------------
// One draw, executed by a 16-lane group: gather the record, x.w, gradient,
// gradient-memory update, scatter of x*gc into Dt.  K == 1: the gradient memory
// is claimed, read and updated by ONE atomic exchange (a repeated draw reads back
// the value just stored, so its gc is exactly 0).  K > 1: an int claim per
// sample, then plain loads/stores.  kLds: Dt is a workgroup-private LDS copy of D
// (ds_add_f64), else the global D (global_atomic_add_f64).
// gc[] returns the draw's gradient change on lane 0 of the group, 0 elsewhere.
// --------------------------------------------------------------------------
// wsrc: the coefficients the draw is evaluated against (d.w, or a virtual shard's replica)
template <int KMAX, bool kLds>
__device__ __forceinline__ void saga_draw(const SagaDev& d, const uint32_t s, const int gl,
                                          const int batch_id, const double (&bk)[KMAX], double* Dt,
                                          double (&gc)[KMAX], const double* wsrc) {
  const int K = KMAX == 1 ? 1 : d.K;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) gc[k] = 0.0;
  const char* base = d.rec + (size_t)s * d.rec_stride;

  // independent of the row (K > 1): claim and old gradient memory
  int prev = batch_id;
  double mold[KMAX];
  if (KMAX > 1) {
    if (gl == 0)
      prev = __hip_atomic_exchange(d.claim + s, batch_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int k = 0; k < KMAX; ++k) mold[k] = (k < K) ? d.M[k + (int64_t)s * K] : 0.0;
  }

  const double y0 = *reinterpret_cast<const double*>(base);
  const int nnz = *reinterpret_cast<const int*>(base + 8);
  const int ovf = *reinterpret_cast<const int*>(base + 12);
  const int cnt0 = nnz < d.rec_cap ? nnz : d.rec_cap;
  const bool has_tail = nnz > cnt0 || cnt0 > kGroup;   // overflow records or a wide main record

  double acc[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) acc[k] = 0.0;

  // first (usually only) chunk of the row stays in registers for the scatter
  int64_t jf = -1;
  double vf = 0.0;
  if (gl < cnt0) {
    jf = reinterpret_cast<const int*>(base + 16)[gl];
    vf = reinterpret_cast<const double*>(base + d.rec_val_off)[gl];
    const double* wj = wsrc + jf * K;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) acc[k] += vf * wj[k];
  }
  if (has_tail) {
    row_for_each<kGroup, kGroup>(d, base, nnz, ovf, gl, [&](int64_t j, double v) {
      const double* wj = wsrc + j * K;
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) acc[k] += v * wj[k];
    });
  }

  double lp[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) lp[k] = grp_sum<kGroup>(acc[k]) + bk[k];

  int first;
  if (KMAX == 1) {
    double g0;
    if (d.family == SGDNET_BINOMIAL)
      g0 = 1.0 - y0 - 1.0 / (1.0 + exp(lp[0]));
    else
      g0 = lp[0] - y0;
    double gcv = 0.0;
    if (gl == 0) {
      const double old = __hip_atomic_exchange(m_slot(d, s), g0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      gcv = g0 - old;
    }
    gc[0] = __shfl(gcv, 0, kGroup);
    first = gc[0] != 0.0;
  } else {
    first = __shfl(prev != batch_id ? 1 : 0, 0, kGroup);
    if (first) {
      // gradient: every lane of the group computes the same K values
      double g[KMAX];
      if (d.family == SGDNET_MULTINOMIAL) {
        const double lse = log_sum_exp(lp, K);
        const unsigned cls = (unsigned)(y0 + 0.5);
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
          g[k] = 0.0;
          if (k < K) {
            g[k] = exp(lp[k] - lse);
            if ((unsigned)k == cls) g[k] -= 1.0;
          }
        }
      } else {
        const double* ys = d.y + (int64_t)s * d.Ky;   // mgaussian: Ky == K responses
#pragma unroll
        for (int k = 0; k < KMAX; ++k) g[k] = (k < K) ? lp[k] - ys[k] : 0.0;
      }
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        if (k < K) {
          gc[k] = g[k] - mold[k];
          if (gl == (k & (kGroup - 1))) d.M[k + (int64_t)s * K] = g[k];
        }
      }
    }
  }

  if (first) {
    if (jf >= 0) {
      double* dj = Dt + jf * K;
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K && gc[k] != 0.0) scatter_add<kLds>(dj + k, vf * gc[k]);
    }
    if (has_tail) {
      row_for_each<kGroup, kGroup>(d, base, nnz, ovf, gl, [&](int64_t j, double v) {
        double* dj = Dt + j * K;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
          if (k < K && gc[k] != 0.0) scatter_add<kLds>(dj + k, v * gc[k]);
      });
    }
  }
  if (gl != 0) {
#pragma unroll
    for (int k = 0; k < KMAX; ++k) gc[k] = 0.0;   // count each draw once in the intercept sum
  }
}

// --------------------------------------------------------------------------
// gather, global-scatter form: one draw per 16-lane group, every draw of the
// batch in flight at once (the kernel is a chain of dependent loads stream ->
// record -> w, so parallelism, not per-thread work, hides the HBM latency).
// Scattered fp64 atomics run at ~23 G requests/s chip-wide: 10 per draw at z = 10.
// --------------------------------------------------------------------------
template <int KMAX>
__global__ __launch_bounds__(kBlock) void saga_batch_gather_kernel(SagaDev d, const LamParams* lamp,
                                                                   int64_t t0_in_epoch, int m,
                                                                   int batch_id_offset) {
  const int K = KMAX == 1 ? 1 : d.K;
  const int gl = threadIdx.x & (kGroup - 1);
  const int i = (blockIdx.x * kBlock + threadIdx.x) / kGroup;
  const int64_t t0 = lamp->stream_base + t0_in_epoch;
  const int batch_id = lamp->batch_seq + batch_id_offset;
  double gc[KMAX], bk[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    gc[k] = 0.0;
    bk[k] = k < K ? d.b[k] - (d.standardize ? cw_sum(d, batch_id, k) : 0.0) : 0.0;
  }
  if (d.standardize) cw_clear_next(d, batch_id);
  if (i < m) saga_draw<KMAX, false>(d, d.stream[t0 + i], gl, batch_id, bk, d.D, gc, d.w);
  if (d.fit_intercept || d.standardize) store_d0_partial<KMAX, kBlock>(d, K, batch_id, gc);
}

__global__ __launch_bounds__(256) void pack_compact_kernel(const int64_t* ptr, const int32_t* idx,
                                                           const double* val, const double* y, int64_t n, int E,
                                                           int y_in_tag, char* P, char* Q, uint32_t* meta) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t q0 = ptr[i];
    const int nnz = (int)(ptr[i + 1] - q0);
    char* pb = P + (size_t)i * kCStride;
    double* pv = reinterpret_cast<double*>(pb);
    uint16_t* pid = reinterpret_cast<uint16_t*>(pb + 8 * E);
    for (int e = 0; e < E; ++e) pv[e] = e < nnz ? val[q0 + e] : 0.0;
    for (int e = 0; e < (kCMOff - 8 * E) / 2; ++e) pid[e] = e < E && e < nnz ? (uint16_t)idx[q0 + e] : (uint16_t)0;
    if (!y_in_tag) *reinterpret_cast<double*>(pb + kCYOff) = y[i];
    *reinterpret_cast<double*>(pb + kCMOff) = 0.0;
    uint32_t bits = 0u;
    if (nnz > E) {
      char* qb = Q + (size_t)i * kCStride;
      reinterpret_cast<int*>(qb)[0] = nnz;
      reinterpret_cast<int*>(qb)[1] = 0;
      uint16_t* qid = reinterpret_cast<uint16_t*>(qb + 8);
      double* qv = reinterpret_cast<double*>(qb + 32);
      for (int e = 0; e < kCQ; ++e) {
        qid[e] = E + e < nnz ? (uint16_t)idx[q0 + E + e] : (uint16_t)0;
        qv[e] = E + e < nnz ? val[q0 + E + e] : 0.0;
      }
      bits |= 1u;
    }
    if (y_in_tag && y[i] != 0.0) bits |= 2u;   // the response of a binomial fit rides in cmeta
    if (bits) atomicOr(meta + (i >> 4), bits << (2 * (i & 15)));
  }
}

// gradient memory between the K x n array and the records (a mode change, or the host reading / writing it)
__global__ __launch_bounds__(256) void m_move_kernel(SagaDev d, int to_record) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < d.n; i += (int64_t)gridDim.x * 256) {
    double* r = reinterpret_cast<double*>(d.cP + (size_t)i * kCStride + kCMOff);
    if (to_record) *r = d.M[i];
    else d.M[i] = *r;
  }
}

// --------------------------------------------------------------------------
// gather, LDS-privatised scatter ("LDS staging of the gradient-average slice"):
// a 1024-thread workgroup owns `draws_per_block` consecutive draws and
// accumulates x*gc into a dense LDS copy of D (K*p doubles, ds_add_f64); at the
// end the copy is flushed with line-coalesced global atomics: lanes i..i+7 of a
// wave hit one 64-B line, so a workgroup issues at most K*p/8 atomic requests
// instead of one per non-zero.
// --------------------------------------------------------------------------

// kWLds (K == 1, 2*p doubles fit the CU's LDS): the coefficient snapshot is staged next to the
// accumulator, so the x.w gather -- 64 distinct addresses per wave instruction, which the
// vector-memory address unit serves at about one lane per clock -- becomes ds_read_b64.
// kVS (K == 1, kWLds): virtual shards -- the launch covers the same batch of d.V sample shards;
// workgroup b works for shard b / d.v_bps on that shard's replica of (w, b), its region of the
// sample stream and its own intercept partial.
template <int KMAX, bool kWLds = false, bool kVS = false, int kLanes = kGroup>
__global__ __launch_bounds__(kLdsBlock) void saga_batch_gather_lds_kernel(SagaDev d, const LamParams* lamp,
                                                                          int64_t t0_in_epoch, int m,
                                                                          int batch_id_offset,
                                                                          int draws_per_block) {
  extern __shared__ __attribute__((aligned(16))) double Dl[];
  const int K = KMAX == 1 ? 1 : d.K;
  const int64_t KP = (int64_t)K * d.p;
  __shared__ int ticket_counter;             // work tickets of the compact K == 1 form
  const int vsh = kVS ? (int)blockIdx.x / d.v_bps : 0;          // this workgroup's shard
  const int vblk = kVS ? (int)blockIdx.x - vsh * d.v_bps : (int)blockIdx.x;
  const double* w_src = kVS ? d.vw + (int64_t)vsh * KP : d.w;
  // compact K == 1 form: the sample ids of every wavefront's first two passes are requested before anything else
  constexpr bool kCompactForm = KMAX == 1 && kLanes == kLanes8;
  const bool compact = kCompactForm && d.cP != nullptr;
  K1Compact cg;
  if (threadIdx.x == 0) ticket_counter = compact ? K1Compact::static_tickets() : 0;
  if (compact)
    cg.begin(d, d.stream + lamp->stream_base + t0_in_epoch + (kVS ? (int64_t)vsh * d.v_dps : 0), m, vblk,
             kVS ? d.v_bps : (int)gridDim.x, &ticket_counter);
  PHASE(0);
  // the tables are moved as 16-byte pairs (half the instructions of a double-wise loop: the
  // kernel is bound by the instructions it issues as much as by memory); an odd last element
  // is handled by one thread
  typedef double pair_t __attribute__((ext_vector_type(2)));
  const int64_t KP2 = KP >> 1;
  {
    pair_t* D2 = reinterpret_cast<pair_t*>(Dl);
    for (int64_t i = threadIdx.x; i < KP2; i += kLdsBlock) D2[i] = pair_t{0.0, 0.0};
    if ((KP & 1) && threadIdx.x == 0) Dl[KP - 1] = 0.0;
  }
  if (kWLds) {
    // all loads of a thread in flight before its first LDS store (a plain copy loop waits for
    // every load in turn)
    constexpr int kStage = 8;                   // one round of loads for up to 16 384 coefficients
    double* Wl = Dl + KP + (KP & 1);            // 16-byte aligned
    const pair_t* w2 = reinterpret_cast<const pair_t*>(w_src);
    pair_t* W2 = reinterpret_cast<pair_t*>(Wl);
    for (int64_t i0 = threadIdx.x; i0 < KP2; i0 += (int64_t)kLdsBlock * kStage) {
      pair_t t[kStage];
#pragma unroll
      for (int r = 0; r < kStage; ++r) {
        const int64_t i = i0 + (int64_t)r * kLdsBlock;
        t[r] = i < KP2 ? w2[i] : pair_t{0.0, 0.0};
      }
#pragma unroll
      for (int r = 0; r < kStage; ++r) {
        const int64_t i = i0 + (int64_t)r * kLdsBlock;
        if (i < KP2) W2[i] = t[r];
      }
    }
    if ((KP & 1) && threadIdx.x == 0) Wl[KP - 1] = w_src[KP - 1];
  }
  if (compact) cg.tag_first();                 // the ids have arrived behind the staging loads
  __syncthreads();
  PHASE(1);

  const int gl = threadIdx.x & (kGroup - 1);
  const int group = threadIdx.x / kGroup;
  const int64_t t0 = lamp->stream_base + t0_in_epoch + (kVS ? (int64_t)vsh * d.v_dps : 0);
  const int batch_id = lamp->batch_seq + batch_id_offset;
  const int lo = vblk * draws_per_block;
  const int hi = (lo + draws_per_block < m) ? lo + draws_per_block : m;

  double gct[KMAX], bk[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    gct[k] = 0.0;
    bk[k] = k < K ? (kVS ? d.vb[vsh * K + k] - (d.standardize ? d.vcw[vsh * K + k] : 0.0)
                         : d.b[k] - (d.standardize ? cw_sum(d, batch_id, k) : 0.0))
                  : 0.0;
  }
  if (d.standardize && !kVS) cw_clear_next(d, batch_id);
  constexpr int kGroups = kLdsBlock / kGroup;
  if (KMAX == 1) {
    // K == 1.  8-lane form (both tables in LDS): compact records when the problem has them.
    // 16-lane form: one pass of U = 4 draws per group; the sample ids of the NEXT pass are
    // requested before this pass's records are waited for (a pass is a chain of dependent round
    // trips, ids -> records -> gradient-memory exchange, and this takes the first one off it).
    // (Two software-pipelined half-passes of 2 draws were 2 us slower once the gradient was
    // evaluated once per pass; records one pass ahead as well: DESIGN.md 5, item 9.)
    constexpr int U = 4;
    const double* wv = kWLds ? Dl + KP + (KP & 1) : d.w;
    const uint32_t* sp = d.stream + t0;
    if constexpr (kLanes == kLanes8) {
      if (compact)
        gct[0] = cg.run(d, bk[0], wv, Dl);
      else
        gct[0] = k1_lanes8_draws<kLdsBlock>(d, sp, lo, hi, bk[0], wv, Dl);
    } else if (lo + group < hi) {
      K1Draws<U> A;
      A.load_ids(d, sp, lo + group, hi, kGroups, gl, lo + group);
      for (int i = lo + group; i < hi; i += kGroups * U) {
        A.load_records(d, gl);
        K1IdsOnly<U> N;
        const int in = i + kGroups * U;
        N.valid_any = in < hi;
        if (N.valid_any) N.load(d, sp, in, hi, kGroups, gl, in);
        A.gradient(d, gl, bk[0], wv);
        gct[0] += A.scatter(d, gl, Dl);
        if (N.valid_any) A.take_ids(N);
      }
    }
  } else {
    for (int i = lo + group; i < hi; i += kGroups) {
      double gc[KMAX];
      saga_draw<KMAX, true>(d, d.stream[t0 + i], gl, batch_id, bk, Dl, gc, w_src);
#pragma unroll
      for (int k = 0; k < KMAX; ++k) gct[k] += gc[k];
    }
  }
  PHASE(2);
  __syncthreads();
  PHASE(3);

  // flush the private copy as this workgroup's slab: plain coalesced stores (atomics would
  // cap the flush at the ~1.3 TB/s atomic rate); the sweep sums the slabs in a fixed order
  double* slab = d.slab + (int64_t)blockIdx.x * KP;
  if (!SGD_ABLATE(d, 2)) {
    if ((KP & 1) == 0) {                        // slabs start at multiples of KP doubles: pairs stay aligned
      const pair_t* D2 = reinterpret_cast<const pair_t*>(Dl);
      pair_t* S2 = reinterpret_cast<pair_t*>(slab);
      for (int64_t i = threadIdx.x; i < KP2; i += kLdsBlock) S2[i] = D2[i];
    } else {
      for (int64_t i = threadIdx.x; i < KP; i += kLdsBlock) slab[i] = Dl[i];
    }
  }
  PHASE(4);
  if (kVS) {                                    // one partial per workgroup and class, summed per shard by the sweep
    __shared__ double vpart[kLdsBlock / 64][KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      if (k < K) {
        const double t = wave_sum(gct[k]);
        if ((threadIdx.x & 63) == 0) vpart[threadIdx.x >> 6][k] = t;
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < K) {
      double tot = 0.0;
      for (int wv = 0; wv < kLdsBlock / 64; ++wv) tot += vpart[wv][threadIdx.x];
      d.vd0[(int64_t)blockIdx.x * K + threadIdx.x] = tot;
    }
  } else if (d.fit_intercept || d.standardize) {
    store_d0_partial<KMAX, kLdsBlock>(d, K, batch_id, gct);
  }
  PHASE(5);
}

// --------------------------------------------------------------------------
// Class-lane form for 4 < K <= 16 (multinomial / mgaussian with many classes): inside a
// 16-lane group lane l owns class l and the group walks the row's non-zeros together.  Every
// access to the K-fastest arrays (w, D, g_memory) is then K contiguous doubles per group =
// one or two 128-B requests, instead of K separate requests per non-zero, and x.w needs no
// cross-lane reduction (only the softmax does).
// --------------------------------------------------------------------------
// returns the gradient change of this lane's class (0 on lanes >= K and on repeated draws)
template <bool kLds>
__device__ __forceinline__ double saga_draw_classlane(const SagaDev& d, const uint32_t s, const int gl,
                                                      const int batch_id, const double bl, double* Dt,
                                                      const double* wsrc) {
  const int K = d.K;
  const bool lane_on = gl < K;
  const char* base = d.rec + (size_t)s * d.rec_stride;
  int prev = batch_id;
  if (gl == 0)
    prev = __hip_atomic_exchange(d.claim + s, batch_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const double mold = lane_on ? d.M[gl + (int64_t)s * K] : 0.0;
  const double y0 = *reinterpret_cast<const double*>(base);
  const int nnz = *reinterpret_cast<const int*>(base + 8);
  const int ovf = *reinterpret_cast<const int*>(base + 12);

  double acc = 0.0;
  row_for_each<0, 1>(d, base, nnz, ovf, 0, [&](int64_t j, double v) {
    if (lane_on) acc += v * wsrc[j * K + gl];
  });
  const double lp = acc + bl;

  double g;
  if (d.family == SGDNET_MULTINOMIAL) {
    const double mx = grp_max<kGroup>(lane_on ? lp : -HUGE_VAL);
    const double ssum = grp_sum<kGroup>(lane_on ? exp(lp - mx) : 0.0);
    const double lse = log(ssum) + mx;
    g = exp(lp - lse);
    if ((unsigned)gl == (unsigned)(y0 + 0.5)) g -= 1.0;
  } else {
    g = lp - (lane_on ? d.y[(int64_t)s * d.Ky + gl] : 0.0);   // mgaussian: Ky == K responses
  }
  const int first = __shfl(prev != batch_id ? 1 : 0, 0, kGroup);
  double gc = 0.0;
  if (first && lane_on) {
    gc = g - mold;
    d.M[gl + (int64_t)s * K] = g;
  }
  if (first) {
    row_for_each<0, 1>(d, base, nnz, ovf, 0, [&](int64_t j, double v) {
      if (lane_on && gc != 0.0) scatter_add<kLds>(Dt + j * K + gl, v * gc);
    });
  }
  return gc;
}

// kVS (kLds only; round 3): virtual shards as in saga_batch_gather_lds_kernel -- workgroup b works for shard
// b / d.v_bps on that shard's replica of (w, b), its region of the sample stream and its own intercept partials.
template <bool kLds, bool kVS = false>
__global__ __launch_bounds__(kLds ? kLdsBlock : kBlock) void saga_batch_gather_cl_kernel(
    SagaDev d, const LamParams* lamp, int64_t t0_in_epoch, int m, int batch_id_offset, int draws_per_block) {
  extern __shared__ __attribute__((aligned(16))) double Dl[];
  __shared__ double d0s[16];
  constexpr int kThreads = kLds ? kLdsBlock : kBlock;
  const int K = d.K;
  const int64_t KP = (int64_t)K * d.p;
  const int gl = threadIdx.x & (kGroup - 1);
  const int group = threadIdx.x / kGroup;
  const int vsh = kVS ? (int)blockIdx.x / d.v_bps : 0;
  const int vblk = kVS ? (int)blockIdx.x - vsh * d.v_bps : (int)blockIdx.x;
  const double* w_src = kVS ? d.vw + (int64_t)vsh * KP : d.w;
  const int64_t t0 = lamp->stream_base + t0_in_epoch + (kVS ? (int64_t)vsh * d.v_dps : 0);
  const int batch_id = lamp->batch_seq + batch_id_offset;
  if (kLds)
    for (int64_t i = threadIdx.x; i < KP; i += kThreads) Dl[i] = 0.0;
  if (threadIdx.x < 16) d0s[threadIdx.x] = 0.0;
  __syncthreads();
  double bl = 0.0;
  if (gl < K)
    bl = kVS ? d.vb[vsh * K + gl] - (d.standardize ? d.vcw[vsh * K + gl] : 0.0)
             : d.b[gl] - (d.standardize ? cw_sum(d, batch_id, gl) : 0.0);
  if (d.standardize && !kVS) cw_clear_next(d, batch_id);

  double gct = 0.0;
  if (kLds) {
    const int lo = vblk * draws_per_block;
    const int hi = (lo + draws_per_block < m) ? lo + draws_per_block : m;
    for (int i = lo + group; i < hi; i += kThreads / kGroup)
      gct += saga_draw_classlane<true>(d, d.stream[t0 + i], gl, batch_id, bl, Dl, w_src);
  } else {
    const int i = blockIdx.x * (kThreads / kGroup) + group;
    if (i < m) gct = saga_draw_classlane<false>(d, d.stream[t0 + i], gl, batch_id, bl, d.D, w_src);
  }
  if (gct != 0.0) __hip_atomic_fetch_add(&d0s[gl], gct, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __syncthreads();
  if (kLds) {
    double* slab = d.slab + (int64_t)blockIdx.x * KP;
    for (int64_t i = threadIdx.x; i < KP; i += kThreads) slab[i] = Dl[i];
  }
  if (kVS) {
    if ((int)threadIdx.x < K) d.vd0[(int64_t)blockIdx.x * K + threadIdx.x] = d0s[threadIdx.x];
  } else if ((d.fit_intercept || d.standardize) && (int)threadIdx.x < K) {
    d0_publish(d, batch_id, threadIdx.x, d0s[threadIdx.x]);
  }
}

// ------------------------------ launchers ---------------------------------
int launch_pack_compact(const SagaDev& d, char* P, char* Q, uint32_t* meta, hipStream_t st) {
  SGD_HIP_TRY(hipMemsetAsync(meta, 0, sizeof(uint32_t) * (size_t)((d.n + 15) / 16 + 1), st));
  const int E = compact_entries(d);
  return launch_kernel(pack_compact_kernel, dim3(clamped_grid(d.n, 256, 65536)), dim3(256), 0, 0, st, nullptr, nullptr,
                       d.ptr, d.idx, d.val, d.y, d.n, E, E == 12 ? 1 : 0, P, Q, meta);
}

int launch_m_move(const SagaDev& d, int to_record, hipStream_t st) {
  return launch_kernel(m_move_kernel, dim3(clamped_grid(d.n, 256, 16384)), dim3(256), 0, 0, st, nullptr, nullptr, d,
                       to_record);
}

// ev0/ev1 (optional): dispatch start/stop timestamps of exactly this kernel
// (hipExtLaunchKernelGGL), used by the benchmark's per-kernel timing.
int launch_batch_gather(const SagaDev& d, const BatchPlan& g, LamParams* lam, int64_t t0_in_epoch, int m,
                        int batch_id_offset, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
  if (d.K > 16 && g.form != BatchForm::kBinned && g.form != BatchForm::kDenseClassLane) {
    set_error("batched mode with more than 16 classes needs the binned form (sparse x) or the class-lane form (dense x), "
              "n_classes <= 64; got %d", d.K);
    return SGDNET_EUNSUPPORTED;
  }
  switch (g.form) {
  case BatchForm::kDenseClassLane:
  case BatchForm::kDenseTiled:
  case BatchForm::kDense:
    return launch_dense_gather(d, g, lam, t0_in_epoch, m, batch_id_offset, st, ev0, ev1);
  case BatchForm::kBinned:
    return launch_binned_gather(d, g, lam, t0_in_epoch, m, batch_id_offset, st, ev0, ev1);
  case BatchForm::kLds: {
    const GatherKernel kernel = g.lanes8    ? saga_batch_gather_lds_kernel<1, true, false, kLanes8>
                                : g.w_lds   ? saga_batch_gather_lds_kernel<1, true>
                                : g.kw == 1 ? saga_batch_gather_lds_kernel<1>
                                : g.kw == 4 ? saga_batch_gather_lds_kernel<4>
                                            : saga_batch_gather_cl_kernel<true>;
    return launch_kernel(kernel, dim3(g.grid), dim3(kLdsBlock), g.lds_bytes, g.lanes8 || g.w_lds ? kLdsAll : kLdsCap, st,
                         ev0, ev1, d, lam, t0_in_epoch, m, batch_id_offset, g.draws_per_block);
  }
  case BatchForm::kGlobal:
    if (g.kw != 1 && g.kw != 4)
      return launch_kernel(saga_batch_gather_cl_kernel<false>, dim3(g.grid), dim3(kBlock), 0, 0, st, ev0, ev1, d, lam,
                           t0_in_epoch, m, batch_id_offset, g.draws_per_block);
    return launch_kernel(g.kw == 1 ? saga_batch_gather_kernel<1> : saga_batch_gather_kernel<4>, dim3(g.grid), dim3(kBlock),
                         0, 0, st, ev0, ev1, d, lam, t0_in_epoch, m, batch_id_offset);
  default:
    set_error("internal: launch_batch_gather given a virtual-shard plan");
    return SGDNET_EINVAL;
  }
}

int launch_vs_gather(const SagaDev& d, const BatchPlan& g, LamParams* lam, int64_t t0_in_epoch, int m, hipStream_t st,
                     hipEvent_t ev0, hipEvent_t ev1, int batch_index) {
  if (g.grid / d.V != d.v_bps || g.grid > kD0Slots) {
    set_error("internal: virtual-shard geometry (%d workgroups, %d per shard)", g.grid, d.v_bps);
    return SGDNET_EINVAL;
  }
  // batch_id_offset: 0 for K == 1; 2..16 classes (round 3 sparse, round 4 dense) take the batch's index in the epoch,
  // the first-occurrence claims of a sample are per batch
  if (d.xd) return launch_dense_vs_gather(d, g, lam, t0_in_epoch, m, st, ev0, ev1, batch_index);
  // 2..4 classes: the 16-lane draw of the LDS form against the shard's replica; 5..16 classes: the class-lane form
  const bool k1 = g.kw != 4 && g.kw != 16;
  const GatherKernel kernel = g.kw == 4    ? saga_batch_gather_lds_kernel<4, false, true>
                              : g.kw == 16 ? saga_batch_gather_cl_kernel<true, true>
                              : g.lanes8   ? saga_batch_gather_lds_kernel<1, true, true, kLanes8>
                                           : saga_batch_gather_lds_kernel<1, true, true>;
  return launch_kernel(kernel, dim3(g.grid), dim3(kLdsBlock), g.lds_bytes, k1 ? kLdsAll : kLdsCap, st, ev0, ev1, d, lam,
                       t0_in_epoch, m, k1 ? 0 : batch_index, g.draws_per_block);
}

}  // namespace sgdnet
