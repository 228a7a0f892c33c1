// Batched SAGA, dense x: the wavefront-per-draw gather (LDS table, virtual shards, tiled), the tiled accumulate pass
// and the class-lane gather and sweep of 17..64 classes.
#include "batched_device.hpp"

namespace sgdnet {

// --------------------------------------------------------------------------
// Dense x (src/saga-dense.h) in batched mode: one wavefront per draw.  A sample is p
// contiguous doubles, so the row streams through coalesced 512-byte wave loads; x.w is a
// wave reduction; x*gc goes into the workgroup's LDS copy of D with conflict-free ds_add_f64
// (lane l owns features l, l+64, ...), and the copy leaves as the workgroup's slab exactly as
// in the sparse LDS form, so the sweep kernels are shared.  The second pass over the row (the
// scatter) re-reads it from L1/L2.  Algorithmic bytes per draw: 8p (row) + 8Ky + 16K.
// --------------------------------------------------------------------------

// kVS (K == 1): virtual shards as in the sparse LDS gather -- workgroup b works for shard
// b / d.v_bps on that shard's replica of (w, b) and its region of the sample stream.
// kTiled: K x p tables that fit no LDS.  The kernel stops after the gradient: the gradient change of
// draw i goes to d.gcb[i * K + k] (zero for a repeated sample) and saga_dense_tiled_accumulate_kernel
// forms D = X_batch^T gc feature tile by feature tile.
template <int KMAX, int kThreads = kDenseBlock, bool kVS = false, bool kTiled = false>
__global__ __launch_bounds__(kThreads) void saga_batch_gather_dense_kernel(SagaDev d, const LamParams* lamp,
                                                                           int64_t t0_in_epoch, int m,
                                                                           int batch_id_offset,
                                                                           int draws_per_block) {
  extern __shared__ __attribute__((aligned(16))) double Dl[];
  const int K = KMAX == 1 ? 1 : d.K;
  const int64_t p = d.p, KP = (int64_t)K * p;
  const int vsh = kVS ? (int)blockIdx.x / d.v_bps : 0;
  const int vblk = kVS ? (int)blockIdx.x - vsh * d.v_bps : (int)blockIdx.x;
  const double* w_src = kVS ? d.vw + (int64_t)vsh * KP : d.w;
  if (!kTiled) {
    for (int64_t i = threadIdx.x; i < KP; i += kThreads) Dl[i] = 0.0;
    __syncthreads();
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t t0 = lamp->stream_base + t0_in_epoch + (kVS ? (int64_t)vsh * d.v_dps : 0);
  const int batch_id = lamp->batch_seq + batch_id_offset;
  const int lo = vblk * draws_per_block;
  const int hi = (lo + draws_per_block < m) ? lo + draws_per_block : m;
  double bk[KMAX], gct[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    bk[k] = k < K ? (kVS ? d.vb[vsh * K + k] : d.b[k]) : 0.0;
    gct[k] = 0.0;
  }
  for (int i = lo + wave; i < hi; i += kThreads / 64) {
    const uint32_t s = d.stream[t0 + i];
    const double* xs = d.xd + (int64_t)s * p;
    int prev = batch_id;
    double mold[KMAX];
    if (KMAX > 1) {   // claim + old gradient memory: independent of the row
      if (lane == 0)
        prev = __hip_atomic_exchange(d.claim + s, batch_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
      for (int k = 0; k < KMAX; ++k) mold[k] = k < K ? d.M[k + (int64_t)s * K] : 0.0;
    }
    double acc[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) acc[k] = 0.0;
    // kRowU row chunks per lane requested before the first use (a plain strided loop waits for
    // every load in turn: the trip count is a run-time value)
    constexpr int kRowU = KMAX == 1 ? 8 : 4;
    for (int64_t j0 = lane; j0 < p; j0 += 64 * kRowU) {
      double xv[kRowU];
#pragma unroll
      for (int r = 0; r < kRowU; ++r) {
        const int64_t j = j0 + 64 * r;
        xv[r] = j < p ? xs[j] : 0.0;
      }
#pragma unroll
      for (int r = 0; r < kRowU; ++r) {
        const int64_t j = j0 + 64 * r;
        if (j < p) {
          const double* wj = w_src + j * K;
#pragma unroll
          for (int k = 0; k < KMAX; ++k)
            if (k < K) acc[k] += xv[r] * wj[k];
        }
      }
    }
    double lp[KMAX], g[KMAX], gc[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      lp[k] = wave_sum(acc[k]) + bk[k];
      gc[k] = 0.0;
    }
    bool first;
    if (KMAX == 1) {
      const double y0 = d.y[(int64_t)s * d.Ky];
      g[0] = d.family == SGDNET_BINOMIAL ? 1.0 - y0 - 1.0 / (1.0 + exp(lp[0])) : lp[0] - y0;
      double gcv = 0.0;
      if (lane == 0) {
        const double old = __hip_atomic_exchange(d.M + s, g[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        gcv = g[0] - old;
      }
      gc[0] = __shfl(gcv, 0, 64);
      first = gc[0] != 0.0;
    } else {
      first = __shfl(prev != batch_id ? 1 : 0, 0, 64) != 0;
      if (first) {
        if (d.family == SGDNET_MULTINOMIAL) {
          const double lse = log_sum_exp(lp, K);
          const unsigned cls = (unsigned)(d.y[(int64_t)s * d.Ky] + 0.5);
#pragma unroll
          for (int k = 0; k < KMAX; ++k) {
            g[k] = 0.0;
            if (k < K) {
              g[k] = exp(lp[k] - lse);
              if ((unsigned)k == cls) g[k] -= 1.0;
            }
          }
        } else if (d.family == SGDNET_MGAUSSIAN) {
          const double* ys = d.y + (int64_t)s * d.Ky;
#pragma unroll
          for (int k = 0; k < KMAX; ++k) g[k] = k < K ? lp[k] - ys[k] : 0.0;
        } else {   // not reached: single-response families have K == 1
#pragma unroll
          for (int k = 0; k < KMAX; ++k) g[k] = 0.0;
        }
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
          if (k < K) {
            gc[k] = g[k] - mold[k];
            if (lane == k) d.M[k + (int64_t)s * K] = g[k];
          }
        }
      }
    }
    if (kTiled) {
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K && lane == k) d.gcb[(int64_t)i * K + k] = first ? gc[k] : 0.0;
    }
    if (first) {
      if (!kTiled) {
        for (int64_t j0 = lane; j0 < p; j0 += 64 * kRowU) {
          double xv[kRowU];
#pragma unroll
          for (int r = 0; r < kRowU; ++r) {
            const int64_t j = j0 + 64 * r;
            xv[r] = j < p ? xs[j] : 0.0;
          }
#pragma unroll
          for (int r = 0; r < kRowU; ++r) {
            const int64_t j = j0 + 64 * r;
            if (j < p) {
              double* dj = Dl + j * K;
#pragma unroll
              for (int k = 0; k < KMAX; ++k)
                if (k < K && gc[k] != 0.0) scatter_add<true>(dj + k, xv[r] * gc[k]);
            }
          }
        }
      }
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < KMAX; ++k) gct[k] += gc[k];
      }
    }
  }
  if (!kTiled) {
    __syncthreads();
    double* slab = d.slab + (int64_t)blockIdx.x * KP;
    for (int64_t i = threadIdx.x; i < KP; i += kThreads) slab[i] = Dl[i];
  }
  if (kVS) {                                    // one partial per workgroup and class, summed per shard by the sweep
    __shared__ double vpart[kThreads / 64][KMAX];
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < KMAX; ++k) vpart[wave][k] = gct[k];
    }
    __syncthreads();
    if ((int)threadIdx.x < K) {
      double tot = 0.0;
      for (int wv = 0; wv < kThreads / 64; ++wv) tot += vpart[wv][threadIdx.x];
      d.vd0[(int64_t)blockIdx.x * K + threadIdx.x] = tot;
    }
  } else if (d.fit_intercept) {
    store_d0_partial<KMAX, kThreads>(d, K, batch_id, gct);
  }
}

// --------------------------------------------------------------------------
// Dense x, K x p beyond the LDS table: D = X_batch^T gc by feature tiles.  A workgroup owns 64
// consecutive features (lane <-> feature: every row segment is one 512-B read) and a chunk of the
// batch's draws (blockIdx.y); its four wavefronts take every fourth draw of the chunk, kTileU rows
// requested before the first is used, and meet in LDS in a fixed order.  One atomic add per
// (feature, class, chunk) into d.D -- chunks x K x p atomics per batch instead of m x K x p.
// Sample ids and gradient changes are wave-uniform (scalar loads); rows whose change is zero
// (repeated samples) are not read.
// --------------------------------------------------------------------------
constexpr int kTileU = 8;

template <int KMAX>
__global__ __launch_bounds__(kDenseBlock) void saga_dense_tiled_accumulate_kernel(SagaDev d, const LamParams* lamp,
                                                                                  int64_t t0_in_epoch, int m,
                                                                                  int draws_per_chunk) {
  __shared__ double part[kDenseBlock / 64 - 1][KMAX][kTileF];
  // more than KMAX classes (round 4, 17..64): blockIdx.z takes KMAX of them at a time; KS = the stride of a draw's
  // (and a feature's) class vector, K = the classes of this chunk
  const int KS = KMAX == 1 ? 1 : d.K;
  const int k0 = (int)blockIdx.z * KMAX;
  const int K = KS - k0 < KMAX ? KS - k0 : KMAX;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  constexpr int kWaves = kDenseBlock / 64;
  const int64_t j = (int64_t)blockIdx.x * kTileF + lane;
  const bool live = j < d.p;
  const int64_t t0 = lamp->stream_base + t0_in_epoch;
  const int lo = (int)blockIdx.y * draws_per_chunk;
  const int hi = (lo + draws_per_chunk < m) ? lo + draws_per_chunk : m;
  double acc[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) acc[k] = 0.0;
  for (int i0 = lo + wave; i0 < hi; i0 += kWaves * kTileU) {
    double xv[kTileU];
    bool on[kTileU];
#pragma unroll
    for (int u = 0; u < kTileU; ++u) {
      const int i = i0 + u * kWaves;
      on[u] = false;
      xv[u] = 0.0;
      if (i < hi) {
        const double* gci = d.gcb + (int64_t)i * KS + k0;
        bool any = false;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) any = any || (k < K && gci[k] != 0.0);
        on[u] = any;
        if (any && live) xv[u] = d.xd[(int64_t)d.stream[t0 + i] * d.p + j];
      }
    }
#pragma unroll
    for (int u = 0; u < kTileU; ++u) {
      if (on[u]) {
        const double* gci = d.gcb + (int64_t)(i0 + u * kWaves) * KS + k0;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
          if (k < K) acc[k] += xv[u] * gci[k];
      }
    }
  }
  if (wave > 0) {
#pragma unroll
    for (int k = 0; k < KMAX; ++k) part[wave - 1][k][lane] = acc[k];
  }
  __syncthreads();
  if (wave == 0 && live) {
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      if (k < K) {
        double tot = acc[k];
#pragma unroll
        for (int wv = 0; wv < kWaves - 1; ++wv) tot += part[wv][k][lane];
        if (tot != 0.0) scatter_add<false>(d.D + j * KS + k0 + k, tot);
      }
    }
  }
}

// --------------------------------------------------------------------------
// Dense x with 17..64 classes (round 4; src/saga-dense.h:149-185 in batched form): the class-lane form.  A wavefront
// per draw, lane k = class k: the row arrives 64 features per load (coalesced), feature j's value is handed to all
// lanes through v_readlane and meets row j of w -- K contiguous doubles, one or a few 128-B lines from L2 -- so x.w
// needs no reduction across lanes and only the softmax does.  The kernel stops after the gradient, like the tiled
// form of fewer classes: the gradient change of draw i goes to d.gcb[i * K + k] (zero for a repeated sample),
// saga_dense_tiled_accumulate_kernel<16> forms D = X_batch^T gc sixteen classes at a time (blockIdx.z) and
// saga_dense_cl_sweep_kernel updates a feature's K coefficients per wavefront.
// Algorithmic bytes per draw: 8 p (row, twice: the accumulate pass reads it again) + 8 K p (w, from L2) + 24 K.
// --------------------------------------------------------------------------
__device__ __forceinline__ double lane_value(double v, int src) {   // src is wave-uniform
  const long long q = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)(q & 0xffffffffll), src);
  const int hi = __builtin_amdgcn_readlane((int)(q >> 32), src);
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

__global__ __launch_bounds__(kDenseBlock) void saga_dense_cl_gather_kernel(SagaDev d, const LamParams* lamp,
                                                                           int64_t t0_in_epoch, int m,
                                                                           int batch_id_offset, int draws_per_block) {
  __shared__ double part[kDenseBlock / 64][64];
  const int K = d.K;
  const int64_t p = d.p;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const bool lane_on = lane < K;
  const int kl = lane_on ? lane : 0;                       // idle lanes read class 0 (addresses stay inside the arrays)
  const int64_t t0 = lamp->stream_base + t0_in_epoch;
  const int batch_id = lamp->batch_seq + batch_id_offset;
  const int lo = (int)blockIdx.x * draws_per_block;
  const int hi = (lo + draws_per_block < m) ? lo + draws_per_block : m;
  const double bk = d.b[kl];
  double gct = 0.0;
  for (int i = lo + wave; i < hi; i += kDenseBlock / 64) {
    const uint32_t s = d.stream[t0 + i];
    const double* xs = d.xd + (int64_t)s * p;
    int prev = batch_id;
    if (lane == 0) prev = __hip_atomic_exchange(d.claim + s, batch_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double mold = d.M[kl + (int64_t)s * K];
    double acc = 0.0;
    for (int64_t j0 = 0; j0 < p; j0 += 64) {
      const double xv = j0 + lane < p ? xs[j0 + lane] : 0.0;
      const int cnt = p - j0 < 64 ? (int)(p - j0) : 64;
      const double* wr = d.w + j0 * K + kl;
      for (int e0 = 0; e0 < cnt; e0 += 8) {                // eight rows of w requested before the first is used
        double wv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) wv[u] = e0 + u < cnt ? wr[(int64_t)(e0 + u) * K] : 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (e0 + u < cnt) acc += lane_value(xv, e0 + u) * wv[u];
      }
    }
    const double lp = acc + bk;
    double g;
    if (d.family == SGDNET_MULTINOMIAL) {
      const double mx = wave_max(lane_on ? lp : -HUGE_VAL);
      const double ssum = wave_sum(lane_on ? exp(lp - mx) : 0.0);
      const double lse = log(ssum) + mx;
      g = exp(lp - lse);
      if ((unsigned)lane == (unsigned)(d.y[(int64_t)s * d.Ky] + 0.5)) g -= 1.0;
    } else {                                               // mgaussian: Ky == K responses
      g = lp - d.y[(int64_t)s * d.Ky + kl];
    }
    const bool first = __shfl(prev != batch_id ? 1 : 0, 0, 64) != 0;
    double gc = 0.0;
    if (first && lane_on) {
      gc = g - mold;
      d.M[lane + (int64_t)s * K] = g;
    }
    if (lane_on) d.gcb[(int64_t)i * K + lane] = gc;
    gct += gc;
  }
  if (d.fit_intercept) {                                   // one partial per workgroup and class, summed by the sweep
    part[wave][lane] = gct;
    __syncthreads();
    if ((int)threadIdx.x < K) {
      double tot = 0.0;
#pragma unroll
      for (int wv = 0; wv < kDenseBlock / 64; ++wv) tot += part[wv][threadIdx.x];
      d0_publish(d, batch_id, threadIdx.x, tot);
    }
  }
}

// Dense class-lane form (17..64 classes, saga_dense_cl_gather_kernel): a wavefront per feature, lane k = class k --
// D_j, w_j and G_j are K contiguous doubles each, the group norm is a wavefront sum.  Dense x is standardised
// explicitly, so there is no implicit centring here.
__global__ __launch_bounds__(kBlock) void saga_dense_cl_sweep_kernel(SagaDev d, LamParams* lamp, int tail, int n_parts,
                                                                     int batch_id_offset) {
  __shared__ double sh_d0[64];
  const SweepParams q = load_sweep_params(d, lamp, tail, SweepOverride{0.0, 0.0, 0.0});
  const int K = d.K;
  const int batch_id = lamp->batch_seq + batch_id_offset;
  if (blockIdx.x == 0 && d.fit_intercept) block_d0<kBlock>(d, n_parts, batch_id, sh_d0);
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  const bool on = j < d.p && lane < K;
  const int64_t t = on ? j * K + lane : 0;
  const double raw = on ? d.D[t] : 0.0, w_old = on ? d.w[t] : 0.0, g_old = on ? d.G[t] : 0.0;
  double v = on ? q.r_m * w_old - q.gamma * q.ls_m * g_old - q.gamma * raw : 0.0;
  const double tau = q.beta * q.gamma * q.ls_m;
  if (q.penalty == SGDNET_GROUPLASSO) {                    // penalties.h:61-79
    const double factor = tau / sqrt(wave_sum(v * v));
    v = factor < 1.0 ? v * (1.0 - factor) : 0.0;
  } else if (q.penalty == SGDNET_ELASTICNET) {
    v = soft_threshold(v, tau);
  }
  if (on) {
    d.w[t] = v;
    if (raw != 0.0) {
      d.G[t] = g_old + raw / q.n_d;
      d.D[t] = 0.0;
    }
  }
  if (blockIdx.x == 0) {
    if (d.fit_intercept) sweep_intercept(d, q, sh_d0);
    double* nxt = d0_set(d, batch_id + 1);                 // the next gather may add into it atomically
    for (int i = threadIdx.x; i < kD0Slots * K; i += kBlock) nxt[i] = 0.0;
  }
}

// ------------------------------ launchers ---------------------------------
int launch_dense_gather(const SagaDev& d, const BatchPlan& g, LamParams* lam, int64_t t0_in_epoch, int m,
                        int batch_id_offset, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
  const dim3 grid(g.grid), block(kDenseBlock);
  // accumulate pass of the tiled forms: feature tiles x draw chunks x groups of 16 classes
  const dim3 agrid((unsigned)((d.p + kTileF - 1) / kTileF), (unsigned)g.chunks, (unsigned)((d.K + 15) / 16));
  if (g.form == BatchForm::kDenseClassLane) {
    const int rc = launch_kernel(saga_dense_cl_gather_kernel, grid, block, 0, 0, st, ev0, nullptr, d, lam, t0_in_epoch, m,
                                 batch_id_offset, g.draws_per_block);
    if (rc) return rc;
    return launch_kernel(saga_dense_tiled_accumulate_kernel<16>, agrid, block, 0, 0, st, nullptr, ev1, d, lam,
                         t0_in_epoch, m, g.draws_per_chunk);
  }
  return with_class_width(g.kw, [&](auto kw) {
    constexpr int KW = decltype(kw)::value;
    if (g.form == BatchForm::kDense)
      return launch_kernel(saga_batch_gather_dense_kernel<KW>, grid, block, g.lds_bytes, kLdsCap, st, ev0, ev1, d, lam,
                           t0_in_epoch, m, batch_id_offset, g.draws_per_block);
    const int rc = launch_kernel(saga_batch_gather_dense_kernel<KW, kDenseBlock, false, true>, grid, block, 0, 0, st, ev0,
                                 nullptr, d, lam, t0_in_epoch, m, batch_id_offset, g.draws_per_block);
    if (rc) return rc;
    return launch_kernel(saga_dense_tiled_accumulate_kernel<KW>, agrid, block, 0, 0, st, nullptr, ev1, d, lam,
                         t0_in_epoch, m, g.draws_per_chunk);
  });
}

// virtual shards.  2..16 classes: four wavefronts per workgroup (a draw holds per-class registers), and the batch's index
// in the epoch as batch_id_offset (launch_vs_gather)
int launch_dense_vs_gather(const SagaDev& d, const BatchPlan& g, LamParams* lam, int64_t t0_in_epoch, int m,
                           hipStream_t st, hipEvent_t ev0, hipEvent_t ev1, int batch_index) {
  const GatherKernel kernel = g.kw == 1   ? saga_batch_gather_dense_kernel<1, kDenseVsBlock, true>
                              : g.kw == 4 ? saga_batch_gather_dense_kernel<4, kDenseBlock, true>
                                          : saga_batch_gather_dense_kernel<16, kDenseBlock, true>;
  return launch_kernel(kernel, dim3(g.grid), dim3(g.kw == 1 ? kDenseVsBlock : kDenseBlock), g.lds_bytes, kLdsCap, st, ev0,
                       ev1, d, lam, t0_in_epoch, m, g.kw == 1 ? 0 : batch_index, g.draws_per_block);
}

int launch_dense_cl_sweep(const SagaDev& d, LamParams* lam, int tail, int n_parts, int batch_id_offset, hipStream_t st,
                          hipEvent_t ev0, hipEvent_t ev1) {
  const int grid = (int)((d.p + kBlock / 64 - 1) / (kBlock / 64));
  return launch_kernel(saga_dense_cl_sweep_kernel, dim3(grid < 1 ? 1 : grid), dim3(kBlock), 0, 0, st, ev0, ev1, d, lam,
                       tail, n_parts, batch_id_offset);
}

}  // namespace sgdnet
