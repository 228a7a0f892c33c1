// Batched SAGA, the sweeps of the single-replica forms (element, slab) with the epoch's bookkeeping kernels, and the
// convergence, loss and multi-GPU delta kernels.  The pieces every sweep shares are in batched_device.hpp.
#include "batched_device.hpp"

namespace sgdnet {

// D accumulated by global atomics (saga_batch_gather_kernel).  Ridge / ElasticNet act per
// element: one thread per (class, feature) entry, fully coalesced over the K-fastest arrays.
// GroupLasso needs the column norm: one thread per feature.
template <bool kGrouped>
__global__ __launch_bounds__(kBlock) void saga_batch_sweep_kernel(SagaDev d, LamParams* lamp, int tail,
                                                                  int n_parts, int batch_id_offset,
                                                                  SweepOverride ov) {
  __shared__ double sh_d0[16];
  const SweepParams q = load_sweep_params(d, lamp, tail, ov);
  const int K = d.K;
  const bool need_d0 = d.standardize || (blockIdx.x == 0 && d.fit_intercept);
  const int batch_id = lamp->batch_seq + batch_id_offset;
  if (need_d0) block_d0<kBlock>(d, n_parts, batch_id, sh_d0);
  double cwp[16];
  for (int k = 0; k < K; ++k) cwp[k] = 0.0;
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (kGrouped) {
    if (t < d.p) {
      double* dg = d.D + t * K;
      double dj[16], wn[16];
      const double cj = d.standardize ? d.c[t] : 0.0;
      for (int k = 0; k < K; ++k) {
        dj[k] = dg[k] - (d.standardize ? cj * sh_d0[k] : 0.0);
        dg[k] = 0.0;
      }
      sweep_feature(d, q, t, dj, wn);
      for (int k = 0; k < K; ++k) cwp[k] = cj * wn[k];
    }
  } else if (t < (int64_t)K * d.p) {
    const int64_t j = t / K;
    const int k = (int)(t - j * K);
    const double cj = d.standardize ? d.c[j] : 0.0;
    const double raw = d.D[t];
    const double dk = raw - (d.standardize ? cj * sh_d0[k] : 0.0);
    double v = q.r_m * d.w[t] - q.gamma * q.ls_m * d.G[t] - q.gamma * dk;
    if (q.penalty == SGDNET_ELASTICNET) v = soft_threshold(v, q.beta * q.gamma * q.ls_m);
    d.w[t] = v;
    if (dk != 0.0) d.G[t] += dk / q.n_d;
    if (raw != 0.0) d.D[t] = 0.0;
    // every lane keeps its own class slot so that cw_accumulate's wave_sum stays per class
    for (int kk = 0; kk < K; ++kk) cwp[kk] = kk == k ? cj * v : 0.0;
  }
  if (d.standardize) cw_accumulate<kBlock>(d, batch_id, cwp);
  if (blockIdx.x == 0) {
    if (d.fit_intercept) sweep_intercept(d, q, sh_d0);
    double* nxt = d0_set(d, batch_id + 1);      // the next gather may add into it atomically
    for (int i = threadIdx.x; i < kD0Slots * K; i += kBlock) nxt[i] = 0.0;
  }
}

// D held as per-workgroup slabs (saga_batch_gather_lds_kernel): a block owns F = 32/K
// features; 8 thread groups each sum an eighth of the slabs (coalesced over the features),
// the partial sums meet in LDS in a fixed order, then one thread per feature updates.
__global__ __launch_bounds__(kBlock) void saga_batch_sweep_slab_kernel(SagaDev d, LamParams* lamp, int tail,
                                                                       int n_parts, int batch_id_offset) {
  __shared__ double part[kSlabGroups][kSlabElems];
  __shared__ double sh_d0[16];
  const SweepParams q = load_sweep_params(d, lamp, tail, SweepOverride{0.0, 0.0, 0.0});
  const int K = d.K;
  const bool need_d0 = d.standardize || (blockIdx.x == 0 && d.fit_intercept);
  const int batch_id = lamp->batch_seq + batch_id_offset;
  if (need_d0) block_d0<kBlock>(d, n_parts, batch_id, sh_d0);
  const int F = kSlabElems / K;              // K <= 16
  const int E = F * K;
  const int64_t KP = (int64_t)K * d.p;
  const int e = threadIdx.x % kSlabElems, g = threadIdx.x / kSlabElems;
  const int64_t elem = (int64_t)blockIdx.x * E + e;
  double acc = 0.0;
  if (e < E && elem < KP) {
    const double* sp = d.slab + elem;
    int bidx = g;
    for (; bidx + 3 * kSlabGroups < n_parts; bidx += 4 * kSlabGroups) {   // 4 loads in flight
      const double a0 = sp[(int64_t)bidx * KP], a1 = sp[(int64_t)(bidx + kSlabGroups) * KP];
      const double a2 = sp[(int64_t)(bidx + 2 * kSlabGroups) * KP];
      const double a3 = sp[(int64_t)(bidx + 3 * kSlabGroups) * KP];
      acc += (a0 + a1) + (a2 + a3);
    }
    for (; bidx < n_parts; bidx += kSlabGroups) acc += sp[(int64_t)bidx * KP];
  }
  part[g][e] = acc;
  __syncthreads();
  double cwp[16];
  for (int k = 0; k < K; ++k) cwp[k] = 0.0;
  if ((int)threadIdx.x < F) {
    const int64_t j = (int64_t)blockIdx.x * F + threadIdx.x;
    if (j < d.p) {
      double dj[16], wn[16];
      const double cj = d.standardize ? d.c[j] : 0.0;
      for (int k = 0; k < K; ++k) {
        const int ee = threadIdx.x * K + k;
        double t = 0.0;
        for (int gg = 0; gg < kSlabGroups; ++gg) t += part[gg][ee];
        dj[k] = t - (d.standardize ? cj * sh_d0[k] : 0.0);
      }
      sweep_feature(d, q, j, dj, wn);
      for (int k = 0; k < K; ++k) cwp[k] = cj * wn[k];
    }
  }
  if (d.standardize) cw_accumulate<kBlock>(d, batch_id, cwp);
  if (blockIdx.x == 0) {
    if (d.fit_intercept) sweep_intercept(d, q, sh_d0);
    double* nxt = d0_set(d, batch_id + 1);      // the next gather may add into it atomically
    for (int i = threadIdx.x; i < kD0Slots * K; i += kBlock) nxt[i] = 0.0;
  }
}

// c.w of the current w into the slot set batch `batch_id` will read; clears the other set.
__global__ __launch_bounds__(kBlock) void saga_cw_init_kernel(SagaDev d, const LamParams* lamp) {
  __shared__ double red[kBlock / 64];
  const int K = d.K;
  const int batch_id = lamp->batch_seq;
  for (int i = threadIdx.x; i < 2 * kCwSlots * K; i += kBlock) d.cw[i] = 0.0;
  __syncthreads();
  for (int k = 0; k < K; ++k) {
    double acc = 0.0;
    for (int64_t j = threadIdx.x; j < d.p; j += kBlock) acc += d.c[j] * d.w[k + j * K];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      double tot = 0.0;
      for (int wv = 0; wv < kBlock / 64; ++wv) tot += red[wv];
      d.cw[(size_t)(batch_id & 1) * kCwSlots * K + k] = tot;
    }
    __syncthreads();
  }
}

// Advances the epoch bookkeeping that graph replays read.
__global__ void saga_epoch_end_kernel(LamParams* lamp, int batches) {
  if (threadIdx.x == 0 && blockIdx.x == 0) end_epoch(lamp, batches);
}

// ConvergenceCheck (src/utils.h:240-262): max |w - w_prev| and max |w|, then w_prev = w.
__global__ __launch_bounds__(kBlock) void saga_convergence_kernel(SagaDev d, LamParams* lamp) {
  const int64_t len = (int64_t)d.K * d.p;
  double max_change = 0.0, max_size = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < len; i += (int64_t)gridDim.x * kBlock) {
    const double v = d.w[i];
    max_change = fmax(max_change, fabs(v - d.w_prev[i]));
    max_size = fmax(max_size, fabs(v));
    d.w_prev[i] = v;
  }
  max_change = wave_max(max_change);
  max_size = wave_max(max_size);
  if ((threadIdx.x & 63) == 0) {
    atomic_max_bits(&lamp->max_change_bits, max_change);
    atomic_max_bits(&lamp->max_size_bits, max_size);
  }
}

// Sum of per-sample losses: Deviance / 2 (src/utils.h:304-329) or n * EpochLoss (:199-227).
template <bool kSparse>
__global__ __launch_bounds__(kBlock) void saga_loss_kernel(SagaDev d, LamParams* lamp) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* lps = reinterpret_cast<double*>(smem);   // [groups per block][K]
  const int K = d.K;
  const int gl = threadIdx.x & (kGroup - 1);
  const int gib = threadIdx.x / kGroup;
  const int64_t group = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kGroup;
  const int64_t ngroups = (int64_t)gridDim.x * (kBlock / kGroup);
  double* lp = lps + (size_t)gib * K;
  // implicit centring (saga-sparse.h:276-277): the reference subtracts sum_j w_kj c_j from every
  // sample's linear predictor; it is the same K numbers for all samples, so each workgroup
  // computes them once (per sample it was O(p K): 94 ms per deviance at 500k x 20k x 10)
  double* cw = lps + (size_t)(kBlock / kGroup) * K;
  if (kSparse && d.standardize) {
    __shared__ double red[kBlock / 64];
    for (int k = 0; k < K; ++k) {
      double a = 0.0;
      for (int64_t j = threadIdx.x; j < d.p; j += kBlock) a += d.w[k + j * K] * d.c[j];
      a = wave_sum(a);
      if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
      __syncthreads();
      if (threadIdx.x == 0) {
        double t = 0.0;
        for (int wv = 0; wv < kBlock / 64; ++wv) t += red[wv];
        cw[k] = t;
      }
      __syncthreads();
    }
  }
  double loss = 0.0;
  if (kSparse && K > 1 && K <= kGroup) {
    // several classes of sparse x (round 4): lane k of the group = class k, the group walks the row together -- a non-zero
    // is ONE request for the K contiguous coefficients of its feature instead of K requests of 8 bytes, and the row is
    // read once instead of K times (config 5: 37 -> 9 ms per deviance, a hundred of them along the path)
    const int kl = gl < K ? gl : 0;
    const double off = (gl < K ? d.b[kl] : 0.0) - (d.standardize ? cw[kl] : 0.0);
    for (int64_t s = group; s < d.n; s += ngroups) {
      const int64_t q0 = d.ptr[s], q1 = d.ptr[s + 1];
      double acc = 0.0;
      for (int64_t q = q0; q < q1; q += 4) {
        double xv[4];
        int64_t jv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          xv[u] = q + u < q1 ? d.val[q + u] : 0.0;
          jv[u] = q + u < q1 ? (int64_t)d.idx[q + u] : 0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc += xv[u] * d.w[kl + jv[u] * K];
      }
      if (gl < K) lp[gl] = acc + off;
      __builtin_amdgcn_wave_barrier();
      if (gl == 0) loss += family_loss(d.family, K, lp, d.y + s * d.Ky);
      __builtin_amdgcn_wave_barrier();
    }
    loss = wave_sum(loss);
    if ((threadIdx.x & 63) == 0 && loss != 0.0) atomic_add_f64(&lamp->loss_acc, loss);
    return;
  }
  for (int64_t s = group; s < d.n; s += ngroups) {
    for (int k = 0; k < K; ++k) {
      double acc = 0.0;
      if (kSparse) {
        for (int64_t q = d.ptr[s] + gl; q < d.ptr[s + 1]; q += kGroup)
          acc += d.val[q] * d.w[k + (int64_t)d.idx[q] * K];
      } else {
        for (int64_t j = gl; j < d.p; j += kGroup) acc += d.xd[s * d.p + j] * d.w[k + j * K];
      }
      acc = grp_sum<kGroup>(acc);
      if (gl == 0) lp[k] = acc - (kSparse && d.standardize ? cw[k] : 0.0) + d.b[k];
    }
    __builtin_amdgcn_wave_barrier();
    if (gl == 0) loss += family_loss(d.family, K, lp, d.y + s * d.Ky);
    __builtin_amdgcn_wave_barrier();
  }
  loss = wave_sum(loss);
  if ((threadIdx.x & 63) == 0 && loss != 0.0) atomic_add_f64(&lamp->loss_acc, loss);
}

// Multi-GPU merge helpers.  Layout: [dG (Kp) | dw (Kp) | dgb (K) | db (K)].
__global__ __launch_bounds__(kBlock) void saga_delta_export_kernel(SagaDev d, const double* ref,
                                                                   double* out, double weight) {
  const int64_t KP = (int64_t)d.K * d.p;
  const int64_t len = 2 * KP + 2 * d.K;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < len; i += (int64_t)gridDim.x * kBlock) {
    double cur;
    if (i < KP) cur = d.G[i];
    else if (i < 2 * KP) cur = d.w[i - KP];
    else if (i < 2 * KP + d.K) cur = d.gb[i - 2 * KP];
    else cur = d.b[i - 2 * KP - d.K];
    out[i] = weight * (cur - ref[i]);
  }
}

// the merged state also becomes the new reference (the next local run's snapshot)
__global__ __launch_bounds__(kBlock) void saga_delta_apply_kernel(SagaDev d, double* ref, const double* merged,
                                                                  double w_weight) {
  const int64_t KP = (int64_t)d.K * d.p;
  const int64_t len = 2 * KP + 2 * d.K;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < len; i += (int64_t)gridDim.x * kBlock) {
    const bool coef = (i >= KP && i < 2 * KP) || i >= 2 * KP + d.K;
    const double v = ref[i] + (coef ? w_weight : 1.0) * merged[i];
    ref[i] = v;
    if (i < KP) d.G[i] = v;
    else if (i < 2 * KP) d.w[i - KP] = v;
    else if (i < 2 * KP + d.K) d.gb[i - 2 * KP] = v;
    else d.b[i - 2 * KP - d.K] = v;
  }
}

// ------------------------------ launchers ---------------------------------
int launch_cw_init(const SagaDev& d, const LamParams* lam, hipStream_t st) {
  return launch_kernel(saga_cw_init_kernel, dim3(1), dim3(kBlock), 0, 0, st, nullptr, nullptr, d, lam);
}

int launch_batch_sweep(const SagaDev& d, const BatchPlan& g, LamParams* lam, int penalty, int tail, int batch_id_offset,
                       hipStream_t st, hipEvent_t ev0, hipEvent_t ev1, double ov_r, double ov_ls, double ov_m) {
  // synchronous sharded mode (ov_m > 0): the slots were summed across ranks whose gather grids
  // may differ by one workgroup, so all of them are read (unused slots are zero)
  const int n_parts = ov_m > 0.0 ? kD0Slots : (g.grid < kD0Slots ? g.grid : kD0Slots);
  const SweepOverride ov{ov_r, ov_ls, ov_m};
  switch (g.form) {
  case BatchForm::kBinned:
    return launch_binned_sweep(d, g, lam, penalty, tail, n_parts, batch_id_offset, st, ev0, ev1);
  case BatchForm::kDenseClassLane:
    return launch_dense_cl_sweep(d, lam, tail, n_parts, batch_id_offset, st, ev0, ev1);
  case BatchForm::kLds:
  case BatchForm::kDense: {
    const int F = kSlabElems / d.K;
    const int grid = (int)((d.p + F - 1) / F);
    return launch_kernel(saga_batch_sweep_slab_kernel, dim3(grid < 1 ? 1 : grid), dim3(kBlock), 0, 0, st, ev0, ev1, d, lam,
                         tail, g.grid, batch_id_offset);
  }
  default: {   // the global-atomic gather and the tiled dense form
    const bool grouped = penalty == SGDNET_GROUPLASSO;   // a thread per feature; else per (class, feature) entry
    const int grid = (int)(((grouped ? 1 : (int64_t)d.K) * d.p + kBlock - 1) / kBlock);
    return launch_kernel(grouped ? saga_batch_sweep_kernel<true> : saga_batch_sweep_kernel<false>,
                         dim3(grid < 1 ? 1 : grid), dim3(kBlock), 0, 0, st, ev0, ev1, d, lam, tail, n_parts,
                         batch_id_offset, ov);
  }
  }
}

int launch_epoch_end(LamParams* lam, int batches, hipStream_t st) {
  return launch_kernel(saga_epoch_end_kernel, dim3(1), dim3(64), 0, 0, st, nullptr, nullptr, lam, batches);
}

int launch_convergence(const SagaDev& d, LamParams* lam, hipStream_t st) {
  return launch_kernel(saga_convergence_kernel, dim3(clamped_grid((int64_t)d.K * d.p, kBlock * 4, 1024)), dim3(kBlock), 0,
                       0, st, nullptr, nullptr, d, lam);
}

int launch_loss(const SagaDev& d, LamParams* lam, bool sparse, hipStream_t st) {
  const dim3 grid(clamped_grid(d.n, (kBlock / kGroup) * 8, 4096));
  const size_t lds = sizeof(double) * ((size_t)(kBlock / kGroup) + 1) * (size_t)d.K;
  return launch_kernel(sparse ? saga_loss_kernel<true> : saga_loss_kernel<false>, grid, dim3(kBlock), lds, 0, st, nullptr,
                       nullptr, d, lam);
}

int launch_delta_export(const SagaDev& d, const double* ref, double* out, double weight, hipStream_t st) {
  const int64_t len = 2 * (int64_t)d.K * d.p + 2 * d.K;
  return launch_kernel(saga_delta_export_kernel, dim3(clamped_grid(len, kBlock, 2048)), dim3(kBlock), 0, 0, st, nullptr,
                       nullptr, d, ref, out, weight);
}

int launch_delta_apply(const SagaDev& d, double* ref, const double* merged, double w_weight, hipStream_t st) {
  const int64_t len = 2 * (int64_t)d.K * d.p + 2 * d.K;
  return launch_kernel(saga_delta_apply_kernel, dim3(clamped_grid(len, kBlock, 2048)), dim3(kBlock), 0, 0, st, nullptr,
                       nullptr, d, ref, merged, w_weight);
}

}  // namespace sgdnet
