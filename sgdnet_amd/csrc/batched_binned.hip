// Batched SAGA, the binned form of sparse x whose K x p tables fit no LDS: gather+bin and the range sweep, with the
// kernels that size the ranges (column counts, range moments) and refresh the padded copy of w.
#include "batched_device.hpp"

namespace sgdnet {

// --------------------------------------------------------------------------
// Binned form: K x p tables that fit no LDS (config 5: K = 10, p = 100 000 -> 8 MB).
//
// With the scatter accumulator in global memory every non-zero of every draw costs K fp64
// atomics, and those execute at the memory side at a fixed chip-wide byte rate (~1.3 TB/s of
// added bytes, MI355X_MICROARCH.md "Global float atomics"): 800 B per draw at K = 10, z = 10,
// i.e. < 1.6 G draws/s whatever the kernel does.  Here the features are cut into R contiguous
// ranges of equal non-zero mass whose K x width slice fits a workgroup's LDS, and a batch runs
// as two kernels without a single global fp atomic:
//
//   gather+bin  (a workgroup per 512 draws, class-lane form): record, x.w from the L2-resident
//               w, gradient, gradient-memory update; the draw's gradient change goes to
//               gcb[t][0..K) and every non-zero becomes a 16-byte entry {t, j, x_tj} staged in
//               LDS, counted per range, and written out behind ONE returning atomic per
//               (workgroup, range) that reserves the run's place in the range's bin;
//   range sweep (a workgroup per range): D[:, lo..hi) in LDS <- sum over the bin's entries of
//               x_tj * gcb[t] (ds_add_f64), then the reference's per-feature update
//               (saga-sparse.h:316-335 / penalties.h via sweep_feature) for its own features,
//               the intercept and centring scalars exactly as in the other sweep kernels.
//
// The entries of a batch (~16 B x z per draw) are written and read once and stay in the
// Infinity Cache between the two kernels; the sums are order-dependent in the last bits like
// every other scatter of this file.
// --------------------------------------------------------------------------
// (BinEntry and the block sizes kBin*, kRange*: batched_geometry.hpp)

__global__ __launch_bounds__(256) void col_count_kernel(const int32_t* idx, int64_t nnz, unsigned* counts) {
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nnz; q += (int64_t)gridDim.x * 256)
    atomicAdd(counts + idx[q], 1u);
}

__global__ __launch_bounds__(256) void wpad_refresh_kernel(const double* w, double* wpad, int K, int KS, int64_t p) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < p * KS) {
    const int64_t j = t / KS;
    const int k = (int)(t - j * KS);
    wpad[t] = k < K ? w[j * K + k] : 0.0;
  }
}

// Second moment of the entries one sample sends to a feature range: sumsq[r] = sum_i c_ir^2 with c_ir the
// non-zeros of sample i inside range r.  A batch of m uniformly drawn samples sends range r a sum of m such
// counts -- mean m * mass_r / n, variance <= m * sumsq[r] / n -- and that, not a Poisson model of independent
// entries, is what the bins have to hold: rows that put 16 entries into one range (block-structured x)
// arrive 16 at a time.  Feature ids ascend inside a row and ranges are contiguous, so a row is a few runs.
__global__ __launch_bounds__(256) void range_moment_kernel(const int64_t* ptr, const int32_t* idx, int64_t n,
                                                           const uint16_t* feat_range, unsigned long long* sumsq) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t q1 = ptr[i + 1];
    int cur = -1;
    unsigned long long c = 0;
    for (int64_t q = ptr[i]; q < q1; ++q) {
      const int r = feat_range[idx[q]];
      if (r != cur) {
        if (c) atomicAdd(sumsq + cur, c * c);
        cur = r;
        c = 0;
      }
      ++c;
    }
    if (c) atomicAdd(sumsq + cur, c * c);
  }
}

int launch_range_moment(const SagaDev& d, const uint16_t* feat_range, unsigned long long* sumsq, int R,
                        hipStream_t st) {
  SGD_HIP_TRY(hipMemsetAsync(sumsq, 0, sizeof(unsigned long long) * (size_t)R, st));
  return launch_kernel(range_moment_kernel, dim3(clamped_grid(d.n, 256, 8192)), dim3(256), 0, 0, st, nullptr, nullptr,
                       d.ptr, d.idx, d.n, feat_range, sumsq);
}

// the padded copy of w the binned gather reads: refreshed at the start of every epoch (w may have
// been set from the host, merged across GPUs or advanced by an exact-mode run in between)
int launch_wpad_refresh(const SagaDev& d, hipStream_t st) {
  if (!d.wpad || d.wpad == d.w) return SGDNET_OK;
  const int64_t tot = d.p * d.KS;
  return launch_kernel(wpad_refresh_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, 0, st, nullptr, nullptr,
                       d.w, d.wpad, d.K, d.KS, d.p);
}

int launch_col_count(const SagaDev& d, int64_t nnz, unsigned* counts, hipStream_t st) {
  SGD_HIP_TRY(hipMemsetAsync(counts, 0, sizeof(unsigned) * (size_t)d.p, st));
  return launch_kernel(col_count_kernel, dim3(clamped_grid(nnz, 256, 8192)), dim3(256), 0, 0, st, nullptr, nullptr, d.idx,
                       nnz, counts);
}

// one entry straight into its bin (staging full: a workgroup that drew unusually long rows)
__device__ __forceinline__ void bin_push_global(const SagaDev& d, const BinEntry& en, unsigned r) {
  const unsigned pos = atomicAdd(d.bin_count + r, 1u);
  const int64_t b0 = d.bin_off[r];
  if ((int64_t)pos < d.bin_off[r + 1] - b0) reinterpret_cast<BinEntry*>(d.bins)[b0 + pos] = en;
  else atomicExch(d.bin_err, 1);
}

// Entries of the row beyond the 32 a group keeps in registers (record slots >= 32 and the overflow
// chain).  Uniform form: every lane sees every entry (x.w); lane form: lane gl takes entries
// gl, gl + 16, ... of every stretch (staging).
// The lane form is row_for_each<2 * kGrp, kGrp> (batched_device.hpp).  The uniform form stays written out here, the
// body of row_for_each<2 * kGrp, 1> at lane 0: through the shared walker the gather's draw loop -- at the register limit
// of a 1024-thread workgroup -- came out with four instructions placed differently, and this kernel's code is kept
// exactly as it was measured.
template <int kGrp, class F>
__device__ __forceinline__ void row_rest_uniform(const SagaDev& d, const char* base, int nnz, int ovf, F f) {
  const int cap = d.rec_cap;
  const int cnt0 = nnz < cap ? nnz : cap;
  const int* ridx = reinterpret_cast<const int*>(base + 16);
  const double* rval = reinterpret_cast<const double*>(base + d.rec_val_off);
  for (int e = 2 * kGrp; e < cnt0; ++e) f((uint32_t)ridx[e], rval[e]);
  int rem = nnz - cnt0;
  while (rem > 0) {
    const char* ob = d.ovf + (size_t)ovf * kOvfStride;
    const int next = reinterpret_cast<const int*>(ob)[0];
    const int c = reinterpret_cast<const int*>(ob)[1];
    const int* oi = reinterpret_cast<const int*>(ob + 8);
    const double* ov = reinterpret_cast<const double*>(ob + 8 + 4 * kOvfCap);
    for (int e = 0; e < c; ++e) f((uint32_t)oi[e], ov[e]);
    rem -= c;
    ovf = next;
  }
}

// What a 16-lane group holds of one draw before it works on it: requested one pass ahead, so the
// record's round trip to HBM overlaps the previous draw's trip to the L2-resident w.
struct BinDraw {
  uint32_t s;
  int i;              // draw index inside the batch, -1: none
  double y0;
  int nnz, ovf;
  int j0;             // record slot gl (whatever the row length: slots past it hold 0)
  double v0;
  int prev;           // lane 0: the claim this draw's exchange returned
};

__device__ __forceinline__ BinDraw bin_fetch(const SagaDev& d, int i, uint32_t s, bool valid, int gl, int batch_id) {
  BinDraw q;
  q.s = s;
  q.i = valid ? i : -1;
  q.y0 = 0.0; q.nnz = 0; q.ovf = 0; q.j0 = 0; q.v0 = 0.0; q.prev = batch_id;
  if (!valid) return q;
  const char* base = d.rec + (size_t)s * d.rec_stride;
  const int cap = d.rec_cap;
  const int* ridx = reinterpret_cast<const int*>(base + 16);
  const double* rval = reinterpret_cast<const double*>(base + d.rec_val_off);
  q.y0 = *reinterpret_cast<const double*>(base);
  const int2 h = *reinterpret_cast<const int2*>(base + 8);
  q.nnz = h.x;
  q.ovf = h.y;
  if (gl < cap) {
    q.j0 = ridx[gl];
    q.v0 = rval[gl];
  }
  if (gl == 0)
    q.prev = __hip_atomic_exchange(d.claim + s, batch_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return q;
}

template <int kGrp>
__device__ __forceinline__ double shfl_d(double v, int src) {
  const long long b = __double_as_longlong(v);
  const int lo = __shfl((int)(b & 0xffffffffll), src, kGrp);
  const int hi = __shfl((int)(b >> 32), src, kGrp);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// kMulti: the multinomial family alone (config 5's) -- the other families' code and their pointers leave the draw loop,
// which sits at the 128-register limit of a 1024-thread workgroup (round 4: two scratch reloads per draw otherwise)
template <int kGrp, bool kMulti = false>
__global__ __launch_bounds__(kBinBlock) void saga_binned_gather_kernel(SagaDev d, const LamParams* lamp,
                                                                       int64_t t0_in_epoch, int m,
                                                                       int batch_id_offset) {
  extern __shared__ __attribute__((aligned(16))) char bsm[];
  __shared__ double d0s[kGrp];
  __shared__ unsigned n_ent;
  __shared__ int n_next;                                 // the next draw of this workgroup nobody has taken yet
  BinEntry* ent = reinterpret_cast<BinEntry*>(bsm);
  unsigned* cnt = reinterpret_cast<unsigned*>(bsm + sizeof(BinEntry) * kBinEntCap);
  unsigned* rbase = cnt + d.R;
  int* rlo = reinterpret_cast<int*>(rbase + d.R);       // R + 1 range boundaries: the range of a feature
  const int K = d.K, KS = d.KS;                          // is found by bisection in LDS, not by a table
                                                         // look-up that costs an L2 request per non-zero
  // ... and the bisection starts from a coarse table (round 4): the range of the first feature of the 2^shift-feature cell
  // the feature lies in, and of the next cell's -- one or two steps instead of log2(R) dependent LDS reads
  unsigned short* rcl = reinterpret_cast<unsigned short*>(rlo + d.R + 1);
  const int cshift = d.coarse_shift;
  const int gl = threadIdx.x & (kGrp - 1);
  const int group = threadIdx.x / kGrp;
  const int lane = threadIdx.x & 63;
  const bool lane_on = gl < K;
  const int64_t t0 = lamp->stream_base + t0_in_epoch;
  const int batch_id = lamp->batch_seq + batch_id_offset;
  PHASE(0);
  for (int r = threadIdx.x; r < d.R; r += kBinBlock) cnt[r] = 0u;
  for (int r = threadIdx.x; r <= d.R; r += kBinBlock) rlo[r] = d.range_lo[r];
  for (int c = threadIdx.x; c <= d.n_coarse; c += kBinBlock) rcl[c] = d.range_coarse[c];
  if (threadIdx.x < kGrp) d0s[threadIdx.x] = 0.0;
  if (threadIdx.x == 0) {
    n_ent = 0u;
    n_next = (int)blockIdx.x * kBinDraws;
  }
  __syncthreads();
  const double bl = lane_on ? d.b[gl] - (d.standardize ? cw_sum(d, batch_id, gl) : 0.0) : 0.0;
  if (d.standardize) cw_clear_next(d, batch_id);
  auto range_of = [&](int j) {
    const int c = j >> cshift;
    int a = rcl[c], b = rcl[c + 1] + 1;       // rlo[a] <= j < rlo[b]
    while (b - a > 1) {
      const int mid = (a + b) >> 1;
      if (j >= rlo[mid]) a = mid; else b = mid;
    }
    return (unsigned)a;
  };

  // stage one entry per active lane: the slots of a wavefront's entries come from one LDS atomic;
  // the staged copy carries its range in the upper 12 bits of the draw index (batch <= 2^20)
  auto stage = [&](bool active, int i, uint32_t j, double v, unsigned r) {
    const unsigned long long mask = __ballot(active);
    if (mask == 0ull) return;
    const int leader = __ffsll((long long)mask) - 1;
    unsigned slot0 = 0u;
    if (lane == leader) slot0 = atomicAdd(&n_ent, (unsigned)__popcll(mask));
    slot0 = (unsigned)__shfl((int)slot0, leader, 64);
    if (!active) return;
    const unsigned slot = slot0 + (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
    if (slot < (unsigned)kBinEntCap) {
      ent[slot] = BinEntry{(uint32_t)i | (r << 20), j, v};
      atomicAdd(cnt + r, 1u);
    } else {
      bin_push_global(d, BinEntry{(uint32_t)i, j, v}, r);
    }
  };

  PHASE(1);
  // Draws are handed out wavefront by wavefront (round 4): a wavefront takes the next 64 / kGrp draws of the workgroup
  // from an LDS counter, two takes ahead of the one it works on (sample id and record stay requested a pass ahead).
  // Rows differ in length and in how their entries stage, and with a fixed share per group the workgroup's barrier
  // waited 10 us of a 53 us loop for its slowest wavefront.  The four groups of a wavefront stay together, so the
  // ballots of stage() remain wave-wide.
  constexpr int kGpw = 64 / kGrp;
  const int lo = blockIdx.x * kBinDraws;
  const int hi = (lo + kBinDraws < m) ? lo + kBinDraws : m;
  (void)group;
  auto take = [&]() -> int {
    int b = 0;
    if (lane == 0) b = atomicAdd(&n_next, kGpw);
    return __builtin_amdgcn_readfirstlane(b) + lane / kGrp;
  };
  double gct = 0.0;
  int i = take();
  int i_nxt = take();
  uint32_t s_nxt = i_nxt < hi ? d.stream[t0 + i_nxt] : 0u;
  BinDraw cur = bin_fetch(d, i, i < hi ? d.stream[t0 + i] : 0u, i < hi, gl, batch_id);
  while (i - lane / kGrp < hi) {                        // (the wavefront's first draw: the same for all its lanes)
    const int i_nn = take();
    const uint32_t s_nn = i_nn < hi ? d.stream[t0 + i_nn] : 0u;
    const BinDraw nxt = bin_fetch(d, i_nxt, s_nxt, i_nxt < hi, gl, batch_id);
    // the class index of this lane, opaque to the compiler inside the loop: it otherwise keeps (array + 8 gl) of every
    // K-fastest array in a register pair across the loop, and the loop is at the 128-register limit (spills reloaded
    // per draw behind s_waitcnt vmcnt(0), i.e. behind the prefetched record)
    int glo = gl;
    asm volatile("" : "+v"(glo));
    // ---- the current draw ----
    const bool have = cur.i >= 0;
    const int cap = d.rec_cap;
    const int cnt0 = cur.nnz < cap ? cur.nnz : cap;
    const int creg = cnt0 < 2 * kGrp ? cnt0 : 2 * kGrp;
    const bool rest = have && (cur.nnz > creg);
    const char* base = d.rec + (size_t)cur.s * d.rec_stride;
    // x . w: the feature ids sit in the group's registers, so the K-contiguous reads of w are all
    // requested before the first one is used
    const unsigned r0 = range_of(cur.j0);
    const double mold = (have && lane_on) ? d.M[glo + (int64_t)cur.s * K] : 0.0;
    double acc = 0.0;
#pragma unroll
    for (int e0 = 0; e0 < kGrp; e0 += kBinW) {
      if (e0 > 0 && !__any(have && creg > e0)) break;
      double wv[kBinW];
#pragma unroll
      for (int e = 0; e < kBinW; ++e) {
        int j = __shfl(cur.j0, e0 + e, kGrp);
        // (timing only, -DSGDNET_EXPERIMENTS: every coefficient row from a 1 MB window -- an upper bound of what
        //  feature ranges held in one XCD's L2 could buy: profiles/r04_c5_xcd_bound.txt)
        if (SGD_ABLATE(d, 32)) j &= 8191;
        wv[e] = (have && e0 + e < creg && lane_on) ? d.wpad[(int64_t)j * KS + glo] : 0.0;
      }
#pragma unroll
      for (int e = 0; e < kBinW; ++e) acc += shfl_d<kGrp>(cur.v0, e0 + e) * wv[e];
    }
    // record slots 16..31 (3 % of the rows at 10 non-zeros per sample): read where they are needed
    int j1 = 0;
    double v1 = 0.0;
    if (__any(have && creg > kGrp)) {
      if (have && kGrp + gl < creg) {
        j1 = reinterpret_cast<const int*>(base + 16)[kGrp + gl];
        v1 = reinterpret_cast<const double*>(base + d.rec_val_off)[kGrp + gl];
      }
      for (int e = 0; e < kGrp; ++e) {
        const int j = __shfl(j1, e, kGrp);
        const double v = shfl_d<kGrp>(v1, e);
        if (have && kGrp + e < creg && lane_on) acc += v * d.wpad[(int64_t)j * KS + glo];
      }
    }
    if (rest)
      row_rest_uniform<kGrp>(d, base, cur.nnz, cur.ovf, [&](uint32_t j, double v) {
        if (lane_on) acc += v * d.wpad[(int64_t)j * KS + glo];
      });
    const double lp = acc + bl;
    double g;
    if (kMulti || d.family == SGDNET_MULTINOMIAL) {
      // softmax as exp(lp - max) / sum: the same number as families.h:235-260's exp(lp - logsumexp) up to rounding
      // (batched parity is a 1e-9 tolerance), one exp and no log per class lane, and none of the log's sixteen
      // constant registers in a loop that sits at the register limit
      const double mx = grp_max<kGrp>(lane_on ? lp : -HUGE_VAL);
      const double ex = lane_on ? exp(lp - mx) : 0.0;
      g = ex / grp_sum<kGrp>(ex);
      if ((unsigned)gl == (unsigned)(cur.y0 + 0.5)) g -= 1.0;
    } else if (d.family == SGDNET_BINOMIAL) {
      g = 1.0 - cur.y0 - 1.0 / (1.0 + exp(lp));
    } else {
      g = lp - ((have && lane_on) ? d.y[(int64_t)cur.s * d.Ky + glo] : 0.0);
    }
    // a repeat inside the batch sees the same snapshot: gradient change 0, nothing to stage
    const bool first = have && (__shfl(cur.prev != batch_id ? 1 : 0, 0, kGrp) != 0);
    if (first && lane_on) {
      const double gc = g - mold;
      d.M[glo + (int64_t)cur.s * K] = g;
      d.gcb[(int64_t)cur.i * KS + glo] = gc;
      gct += gc;
    }
    stage(first && gl < creg, cur.i, (uint32_t)cur.j0, cur.v0, r0);
    if (__any(first && creg > kGrp)) {
      const bool a1 = first && kGrp + gl < creg;
      const unsigned r1 = range_of(j1);
      stage(a1, cur.i, (uint32_t)j1, v1, r1);
    }
    if (first && rest)
      row_for_each<2 * kGrp, kGrp>(d, base, cur.nnz, cur.ovf, gl, [&](uint32_t j, double v) {
        stage(true, cur.i, j, v, range_of((int)j));
      });
    cur = nxt;
    i = i_nxt;
    i_nxt = i_nn;
    s_nxt = s_nn;
  }
  PHASE(2);
  if (gct != 0.0) __hip_atomic_fetch_add(&d0s[gl], gct, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __syncthreads();
  PHASE(3);
  // reserve this workgroup's run in every bin it has entries for, then place the entries
  // (rbase[r] becomes the ABSOLUTE entry index of the run's start, 0xffffffff if the bin is full)
  for (int r = threadIdx.x; r < d.R; r += kBinBlock) {
    const unsigned c = cnt[r];
    unsigned at = 0xffffffffu;
    if (c) {
      const unsigned pos = atomicAdd(d.bin_count + r, c);
      const int64_t b0 = d.bin_off[r], room = d.bin_off[r + 1] - b0;
      if ((int64_t)pos + c <= room) at = (unsigned)(b0 + pos);
      else atomicExch(d.bin_err, 1);
    }
    rbase[r] = at;
    cnt[r] = 0u;
  }
  __syncthreads();
  PHASE(4);
  const unsigned staged = n_ent < (unsigned)kBinEntCap ? n_ent : (unsigned)kBinEntCap;
  static_assert(sizeof(BinEntry) == sizeof(uint4), "an entry moves as one 16-byte vector");
  for (unsigned e = threadIdx.x; e < staged; e += kBinBlock) {
    const uint4 en = reinterpret_cast<const uint4*>(ent)[e];  // (a modified struct copy went through scratch memory here)
    const unsigned r = en.x >> 20;
    const unsigned at = rbase[r];
    const unsigned k = atomicAdd(cnt + r, 1u);
    if (at != 0xffffffffu) reinterpret_cast<uint4*>(d.bins)[(size_t)at + k] = make_uint4(en.x & 0xfffffu, en.y, en.z, en.w);
  }
  if ((d.fit_intercept || d.standardize) && (int)threadIdx.x < K)
    d0_publish(d, batch_id, threadIdx.x, d0s[threadIdx.x]);
  PHASE(5);
}

// kGrouped: the group-lasso update (a feature's K coefficients in one thread's registers); false: ridge / elastic net
// per element -- that instantiation (config 5's) keeps nothing in scratch memory: a kernel that declares a private
// segment pays for its set-up at every dispatch, and this one is launched 382 times per epoch
template <int kGrp, bool kGrouped>
__global__ __launch_bounds__(kRangeBlock) void saga_binned_sweep_kernel(SagaDev d, LamParams* lamp, int tail,
                                                                        int n_parts, int batch_id_offset) {
  extern __shared__ __attribute__((aligned(16))) double Dl[];
  __shared__ double sh_d0[kGrp];
  __shared__ double sh_cw[kGrp];
  const SweepParams q = load_sweep_params(d, lamp, tail, SweepOverride{0.0, 0.0, 0.0});
  const int K = d.K;
  const int r = blockIdx.x;
  const int batch_id = lamp->batch_seq + batch_id_offset;
  if (r == d.R) {
    // the extra workgroup: intercept update and the reset of the next batch's accumulator slots.
    // (Summing the gather's partials class by class takes ~9 us; inside a range's workgroup that
    // was the tail every launch waited for.)
    if (d.fit_intercept) {
      block_d0<kRangeBlock>(d, n_parts, batch_id, sh_d0);
      sweep_intercept(d, q, sh_d0);
    }
    double* nxt = d0_set(d, batch_id + 1);
    for (int i = threadIdx.x; i < kD0Slots * K; i += kRangeBlock) nxt[i] = 0.0;
    return;
  }
  const int lo = d.range_lo[r], hi = d.range_lo[r + 1];
  const int E = (hi - lo) * K;
  const bool need_d0 = d.standardize != 0;
  // ---- the bin's entries into the LDS slice ----
  // A 16-lane group takes 16 consecutive entries with one coalesced load (lane q holds entry q),
  // then works through them with lane = class: the K-contiguous gradient changes of the 16 draws
  // are requested together, the products go into the slice with ds_add_f64.  The next 16 entries
  // are requested before the current ones are used.
  const int gl = threadIdx.x & (kGrp - 1);
  const int group = threadIdx.x / kGrp;
  constexpr int kGrps = kRangeBlock / kGrp;
  constexpr int kEnt = 16;                        // entries a group takes per round (held by its first 16 lanes)
  unsigned cntb = d.bin_count[r];
  const int64_t b0 = d.bin_off[r], bcap = d.bin_off[r + 1] - b0;
  if ((int64_t)cntb > bcap) cntb = (unsigned)bcap;
  const BinEntry* bin = reinterpret_cast<const BinEntry*>(d.bins) + b0;
  const bool lane_on = gl < K;
  const BinEntry none{0u, (uint32_t)lo, 0.0};
  PHASE(6);
  unsigned e0 = (unsigned)group * kEnt;
  BinEntry mine = (gl < kEnt && e0 + gl < cntb) ? bin[e0 + gl] : none;
  for (int i = threadIdx.x; i < E; i += kRangeBlock) Dl[i] = 0.0;
  if (need_d0) block_d0<kRangeBlock>(d, n_parts, batch_id, sh_d0);
  __syncthreads();
  PHASE(7);
  for (; e0 < cntb; e0 += kGrps * kEnt) {
    const unsigned en = e0 + kGrps * kEnt;
    const BinEntry nxt = (gl < kEnt && en + gl < cntb) ? bin[en + gl] : none;
    double gq[kEnt];
#pragma unroll
    for (int qq = 0; qq < kEnt; ++qq) {
      int t = __shfl((int)mine.t, qq, kGrp);
      if (SGD_ABLATE(d, 64)) t &= 8191;         // (timing only: every gradient-change row from a 1 MB window)
      gq[qq] = (lane_on && e0 + qq < cntb) ? d.gcb[(int64_t)t * d.KS + gl] : 0.0;
    }
#pragma unroll
    for (int qq = 0; qq < kEnt; ++qq) {
      const int j = __shfl((int)mine.j, qq, kGrp);
      const double x = shfl_d<kGrp>(mine.x, qq);
      if (lane_on && e0 + qq < cntb) scatter_add<true>(Dl + (j - lo) * K + gl, x * gq[qq]);
    }
    mine = nxt;
  }
  PHASE(8);
  __syncthreads();
  PHASE(9);
  if (threadIdx.x == 0) d.bin_count[r] = 0u;                 // the next batch fills the bin again
  // ---- per-feature update of this range ----
  if (kGrouped) {
    double cwp[kGrp];
    for (int k = 0; k < K; ++k) cwp[k] = 0.0;
    for (int f = threadIdx.x; f < hi - lo; f += kRangeBlock) {
      const int64_t j = lo + f;
      double dj[kGrp], wn[kGrp];
      const double cj = d.standardize ? d.c[j] : 0.0;
      for (int k = 0; k < K; ++k) dj[k] = Dl[f * K + k] - (d.standardize ? cj * sh_d0[k] : 0.0);
      sweep_feature(d, q, j, dj, wn);
      for (int k = 0; k < K; ++k) cwp[k] += cj * wn[k];
      if (d.wpad != d.w)
        for (int k = 0; k < K; ++k) d.wpad[j * d.KS + k] = wn[k];
    }
    if (d.standardize) cw_accumulate<kRangeBlock>(d, batch_id, cwp);
  } else {
    const double tau = q.beta * q.gamma * q.ls_m, gls = q.gamma * q.ls_m;
    if (d.standardize) {                        // c . w_new of this range, class by class, through the LDS
      if ((int)threadIdx.x < kGrp) sh_cw[threadIdx.x] = 0.0;
      __syncthreads();
    }
    for (int i = threadIdx.x; i < E; i += kRangeBlock) {
      const int f = i / K, k = i - f * K;
      const int64_t t = (int64_t)lo * K + i;
      const double cj = d.standardize ? d.c[lo + f] : 0.0;
      const double dk = Dl[i] - (d.standardize ? cj * sh_d0[k] : 0.0);
      double v = q.r_m * d.w[t] - gls * d.G[t] - q.gamma * dk;
      if (q.penalty == SGDNET_ELASTICNET) v = soft_threshold(v, tau);
      d.w[t] = v;
      if (d.wpad != d.w) d.wpad[(int64_t)(lo + f) * d.KS + k] = v;
      if (dk != 0.0) d.G[t] += dk / q.n_d;
      if (d.standardize && cj * v != 0.0)
        __hip_atomic_fetch_add(&sh_cw[k], cj * v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    if (d.standardize) {                        // (as cw_accumulate: into the next batch's c.w slots)
      __syncthreads();
      if ((int)threadIdx.x < K) {
        const double tot = sh_cw[threadIdx.x];
        double* set = d.cw + (size_t)((batch_id + 1) & 1) * kCwSlots * K;
        if (tot != 0.0) atomic_add_f64(set + (blockIdx.x % kCwSlots) * K + threadIdx.x, tot);
      }
    }
  }
  PHASE(10);
}

// ------------------------------ launchers ---------------------------------
int launch_binned_gather(const SagaDev& d, const BatchPlan& g, LamParams* lam, int64_t t0_in_epoch, int m,
                         int batch_id_offset, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
  void (*kernel)(SagaDev, const LamParams*, int64_t, int, int) =
      g.kw == 64                          ? saga_binned_gather_kernel<64>
      : d.family == SGDNET_MULTINOMIAL ? saga_binned_gather_kernel<16, true>
                                          : saga_binned_gather_kernel<16>;
  return launch_kernel(kernel, dim3(g.grid), dim3(kBinBlock), g.lds_bytes, kLdsAll, st, ev0, ev1, d, lam, t0_in_epoch, m,
                       batch_id_offset);
}

int launch_binned_sweep(const SagaDev& d, const BatchPlan& g, LamParams* lam, int penalty, int tail, int n_parts,
                        int batch_id_offset, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
  const bool grouped = penalty == SGDNET_GROUPLASSO;
  void (*kernel)(SagaDev, LamParams*, int, int, int) =
      g.kw == 64 ? (grouped ? saga_binned_sweep_kernel<64, true> : saga_binned_sweep_kernel<64, false>)
                 : (grouped ? saga_binned_sweep_kernel<16, true> : saga_binned_sweep_kernel<16, false>);
  return launch_kernel(kernel, dim3(d.R + 1), dim3(kRangeBlock), sizeof(double) * (size_t)d.K * (size_t)d.range_max,
                       (int)kRangeLdsBytes, st, ev0, ev1, d, lam, tail, n_parts, batch_id_offset);
}

}  // namespace sgdnet
