// Batched SAGA, the K == 1 machinery that the LDS-privatised gather (saga_batched.hip) and the fused epoch kernel
// (batched_shards.hip) share: the 16-lane pipeline, the 8-lane form, compact records and the work tickets.
#pragma once

#include "batched_device.hpp"
#include "r_rng_word.hpp"

namespace sgdnet {

// --------------------------------------------------------------------------
// K == 1 software pipeline for the LDS-privatised gather: a 16-lane group keeps 2*U
// draws in flight.  The source is ordered in phases (stream -> records -> x.w ->
// gradient -> gradient-memory exchange -> LDS scatter) with no atomic between the
// loads of a phase, so the round trips of every phase overlap.  A record's first
// `cap` slots are always readable (zero padded), so the idx/val loads do not wait
// for the header.
// --------------------------------------------------------------------------

// One pipeline stage set for U draws of a 16-lane group (K == 1).
// --------------------------------------------------------------------------
// K == 1, 8-lane form (records with rec_cap >= 16): an 8-lane group owns FOUR draws per pass
// and every lane holds TWO entries of each (one 8-byte index load, one 16-byte value load), so
// a wavefront carries 32 draws per pass -- twice the records in flight of the 16-lane form for
// the same number of load, exp and exchange instructions.  Lane 2q of the group owns draw q:
// it loads the draw's sample id and the record header (response, nnz, overflow link),
// evaluates the gradient and issues the gradient-memory exchange.  Entries 16.. of a row
// (2.7 % of the rows at 10 non-zeros per row) take the tail path below.
// Unused slots of a record are zero (both packers clear the records), so no per-entry count
// is needed: a zero value contributes nothing and is skipped by the scatter.
// --------------------------------------------------------------------------
constexpr int kLanes8 = 8;
// (kInReg8, the entries of a row held in registers: batched_geometry.hpp)

struct RecHeader {
  double y;
  int nnz;
  int ovf;
};

// All draws lo + g8 + k * (groups * 4) .. of one group; returns the sum of the gradient changes
// of the draws this lane owns.
template <int kThreads>
__device__ __forceinline__ double k1_lanes8_draws(const SagaDev& d, const uint32_t* sp, int lo, int hi, double b0,
                                                  const double* wv, double* Dl) {
  typedef int ipair_t __attribute__((ext_vector_type(2)));
  typedef double dpair_t __attribute__((ext_vector_type(2)));
  constexpr int U = 4;
  constexpr int kG = kThreads / kLanes8;        // groups per workgroup
  constexpr int kStep = kG * U;                 // draws per workgroup pass
  const int gl = threadIdx.x & (kLanes8 - 1);
  const int g8 = threadIdx.x / kLanes8;
  const int q = gl >> 1;                        // the draw of the pass this lane owns / holds x.w of
  const bool is_owner = (gl & 1) == 0;
  const size_t stride = (size_t)d.rec_stride;
  const int val_off = d.rec_val_off;
  double gct = 0.0;
  int i = lo + g8;
  if (i >= hi) return 0.0;
  // sample id of this lane's own draw; draws past the end stand in with draw i (discarded)
  uint32_t s_own = sp[i + q * kG < hi ? i + q * kG : i];
  for (; i < hi; i += kStep) {
    const bool v_own = i + q * kG < hi;
    uint32_t su[U];
#pragma unroll
    for (int u = 0; u < U; ++u) su[u] = (uint32_t)__shfl((int)s_own, 2 * u, kLanes8);
    const RecHeader hd = *reinterpret_cast<const RecHeader*>(d.rec + (size_t)s_own * stride);
    ipair_t jf[U];
    dpair_t vf[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const char* base = d.rec + (size_t)su[u] * stride;
      jf[u] = *reinterpret_cast<const ipair_t*>(base + 16 + 8 * gl);
      vf[u] = *reinterpret_cast<const dpair_t*>(base + val_off + 16 * gl);
    }
    // ids of the next pass: requested before this pass's records are waited for
    const uint32_t s_this = s_own;
    {
      const int in = i + kStep;
      if (in < hi) s_own = sp[in + q * kG < hi ? in + q * kG : in];
    }
    double acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = vf[u].x * wv[jf[u].x] + vf[u].y * wv[jf[u].y];
    const bool own_tail = v_own && hd.nnz > kInReg8;
    const bool any_tail = __ballot(own_tail) != 0;        // wave-uniform
    if (any_tail) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int nz = __shfl(own_tail ? hd.nnz : 0, 2 * u, kLanes8);
        if (nz > kInReg8) {
          const int ov = __shfl(hd.ovf, 2 * u, kLanes8);
          double a = 0.0;
          row_for_each<kInReg8, kLanes8>(d, d.rec + (size_t)su[u] * stride, nz, ov, gl, [&](int64_t j, double v) { a += v * wv[j]; });
          acc[u] += a;
        }
      }
    }
    // merged butterfly: xor 4 halves four values to two, xor 2 to one, xor 1 finishes; draw q's
    // x.w ends up in lanes 2q, 2q+1 of the group
    const bool hi4 = (gl & 4) != 0, hi2 = (gl & 2) != 0;
    const double r0 = (hi4 ? acc[2] : acc[0]) + __shfl_xor(hi4 ? acc[0] : acc[2], 4, kLanes8);
    const double r1 = (hi4 ? acc[3] : acc[1]) + __shfl_xor(hi4 ? acc[1] : acc[3], 4, kLanes8);
    double t = (hi2 ? r1 : r0) + __shfl_xor(hi2 ? r0 : r1, 2, kLanes8);
    t += __shfl_xor(t, 1, kLanes8);
    const double lp = t + b0;
    const double g0 = d.family == SGDNET_BINOMIAL ? 1.0 - hd.y - 1.0 / (1.0 + exp(lp)) : lp - hd.y;
    double gcp = 0.0;
    if (is_owner && v_own) {
      // claim, read and update in ONE returning atomic: a repeated draw of the batch reads back
      // the value just stored (same snapshot, same g0), so its gc is exactly 0
      const double old = __hip_atomic_exchange(m_slot(d, s_this), g0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      gcp = g0 - old;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const double gc = __shfl(gcp, 2 * u, kLanes8);
      if (gc != 0.0) {
        if (vf[u].x != 0.0) scatter_add<true>(Dl + jf[u].x, vf[u].x * gc);
        if (vf[u].y != 0.0) scatter_add<true>(Dl + jf[u].y, vf[u].y * gc);
        if (any_tail) {
          const int nz = __shfl(own_tail ? hd.nnz : 0, 2 * u, kLanes8);
          if (nz > kInReg8) {
            const int ov = __shfl(hd.ovf, 2 * u, kLanes8);
            row_for_each<kInReg8, kLanes8>(d, d.rec + (size_t)su[u] * stride, nz, ov, gl,
                      [&](int64_t j, double v) { scatter_add<true>(Dl + j, v * gc); });
          }
        }
      }
    }
    gct += gcp;
  }
  return gct;
}

// --------------------------------------------------------------------------
// Compact records (K == 1, p <= 65536) with the gradient memory inside.
//
// Round 2's gather read a draw's record and then claimed / read / updated the sample's gradient memory with
// one returning device-scope exchange on a separate 80 MB table.  What the memory system charges for the
// candidates was measured without any compute (scripts/microbench/gather_patterns.hip, profiles/r03b_*,
// r03j_*; a fresh stream segment per repetition): random 128-B lines 24 us per 2^20 draws; line + dependent
// exchange on the separate table 54 us; line + an independent 8-byte load from a second table 45 us (ANY second
// random access costs what the line costs: the fabric serves ~45 G requests/s whatever their size); line + the
// same exchange aimed INTO the line just read 51.6 us; line + a plain 8-byte store into it 43-47 us.  So the
// gradient memory of sample s lives in the last 8 bytes of the sample's own line, and the 0/1 response of a
// binomial fit in a bit beside the long-row bit, which frees the room for a twelfth entry.
//
// The plain store needs to know beforehand which of a batch's repeated draws of a sample carries the change
// (the exchange decides it on the fly: a repeat reads back the value just stored).  That was built and
// measured -- stream_tag_kernel, a bitmap of the shard's samples in LDS, tagged draws `sample | first | long
// | y`: the gather came down to 62-63.5 us per launch alone (from 66), but marking first occurrences is
// 10M LDS atomics + 10M gathers per epoch on CUs that retire about one lane per clock of either: 185 us per
// epoch as one workgroup per shard and batch, 117 + 51 us as eight sub-range workgroups per batch with dense
// bit planes and a combine kernel, 139 us with three sub-ranges storing their words directly (partial-line
// writes), and hidden on the sample-order side stream it took CUs from the gather (62 -> 68 us per launch).
// The exchange INTO the record needs none of it and gives up ~2 us per launch: DESIGN.md 5 "Round 3".
//
//   plane P, 128 B per sample:  [ val[E] : 8 E | id[E] : 2 E (16-bit) | pad | y : 8 at 112 (E = 11) | M : 8 at 120 ]
//       E = 12 for binomial fits (the 0/1 response is a bit of cmeta), 11 otherwise
//   plane Q, 128 B per sample, touched only for rows with more than E entries (21 % / 30 % at 10 per row):
//       [ nnz : 4 | - : 4 | id[12] : 24 | val[12] : 96 ]   entries E .. E + 11
//   entries E + 12 .. of a row are read from the sample-major CSR arrays
//   cmeta, 2 bits per sample: bit 0 = the row has more than E entries, bit 1 = y != 0 (binomial); looked up
//       one pass ahead for sample ids requested two passes ahead, and carried in the id's spare high bits
//
// Lane mapping as before: lanes 0..5 of the 8-lane group hold P's entries 2 slot, 2 slot + 1, lanes 6..7 the
// first four of Q; entries E + 4 .. take the tail path.
// --------------------------------------------------------------------------
constexpr int kCQ = 12;               // entries in plane Q
constexpr int kCYOff = 112;           // response inside plane P (E = 11)
constexpr uint32_t kLongBit = 0x80000000u;
constexpr uint32_t kYBit = 0x20000000u;
// (kCStride, kIdMask: batched_geometry.hpp)
constexpr int kCMOff = 120;

// entries E + 4 .. of a long row
template <class F>
__device__ __forceinline__ void row_tail_compact(const SagaDev& d, uint32_t sid, int nnz, int gl, int E, F f) {
  const char* qb = d.cQ + (size_t)sid * kCStride;
  for (int e = E + 4 + gl; e < nnz; e += kLanes8) {
    if (e < E + kCQ) {
      f((int64_t) reinterpret_cast<const uint16_t*>(qb + 8)[e - E],
        reinterpret_cast<const double*>(qb + 32)[e - E]);
    } else {
      const int64_t q0 = d.ptr[sid];
      f((int64_t)d.idx[q0 + e], d.val[q0 + e]);
    }
  }
}

// Work distribution: a ticket is 32 consecutive draws (one wavefront pass: 8 groups x 4 draws,
// one 128-B line of the sample stream).  A workgroup owns a fixed range of the launch, and its
// 16 wavefronts draw tickets of that range from a counter in LDS: identical shares per
// wavefront left the workgroup waiting for its slowest wavefront (per-pass times vary by tens of
// per cent with the memory system's queues), and a workgroup's time is then the MAXIMUM of 16
// sums of 8 passes instead of their mean.  The LDS counter costs one ds_add_rtn per pass; it is
// used from 4 passes per wavefront (C4 with 8 shards: 0.83 -> 0.79..0.81 ms/epoch, with one shard
// and a single pass per wavefront it only adds latency: 2.08 -> 2.22).
// Tried and removed: handing the last 6-20 % of a launch out ACROSS workgroups from a per-shard
// counter in global memory.  Those tickets serialise on one L2 atomic unit (5-10 ns each) and
// every wavefront reserves three ahead: C4 with 8 shards 1256 -> 1141..1186 epochs/s, with 4
// shards 1016 -> 729; all tickets from a global counter: 160 us per 131 072-draw launch.
constexpr int kTicket = 32;           // draws per wavefront pass

struct TicketSource {
  int* counter;        // LDS, zeroed before the workgroup's barrier
  int lo, hi, m;       // the workgroup's range; m: end of the launch (sentinel)
  int t = 0;
  bool dynamic;
  __device__ __forceinline__ int next() {
    if (!dynamic) {                             // a pass or two per wavefront: nothing to balance
      const int b = lo + (t++ * (kLdsBlock / 64) + (int)(threadIdx.x >> 6)) * kTicket;
      return b < hi ? b : m;
    }
    int b = 0;
    if ((threadIdx.x & 63) == 0)
      b = __hip_atomic_fetch_add(counter, kTicket, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    b = lo + __builtin_amdgcn_readfirstlane(b);
    return b < hi ? b : m;
  }
};

// The K == 1 compact gather of one workgroup over the draws sp[0, m) of its shard-batch.  The kernel runs it in
// three steps so that the first round trips of a workgroup overlap the staging of w into LDS instead of
// following it: begin() (static tickets for every wavefront's first two passes, their sample ids requested)
// before the staging, tag_first() (the first pass's cmeta bits) behind it, run() after the workgroup's barrier.
// (Also requesting the first pass's records before the barrier, with the loop's record loads moved to its end,
// carries one pass's registers across the back edge: 128 VGPRs and 112 bytes of scratch.)
// kRawStream: sp[] may hold the generators' raw words instead of draws (`raw`, wave-uniform; the fused epoch kernel
// over a slot of the sample-order pipeline).  A word becomes a sample id where it is first needed as one, right in
// front of tagged(): in tag_first() for the first pass, one pass ahead in run() for all others.  The stream is only
// read.  Without kRawStream the struct is what it was.
template <bool kRawStream>
struct K1CompactT {
  typedef double dpair_t __attribute__((ext_vector_type(2)));
  static constexpr int U = 4;
  // lane geometry
  int E, in_reg, gl, g, q, slot, id_off, v_off;
  bool y_in_meta, is_owner, in_p, half;
  const char* plane;
  char* P;
  const uint32_t* sp;
  const uint32_t* meta;
  int m;
  TicketSource tk;
  int b_cur, b_nxt;
  uint32_t s_cur, s_nxt;      // s_cur: tagged (long row, response); s_nxt: as read from the stream
  bool raw = false;           // kRawStream: the stream holds raw words
  const double* par = nullptr;  // kRawStream: (n_v, lo_v) of the shard, in LDS: read where a word is converted, not carried

  // a word as read from the stream -> sample id (the expression of rng_convert_kernel, r_rng_device.hip)
  __device__ __forceinline__ uint32_t sample_id(uint32_t x) const {
    if (kRawStream && raw) x = (uint32_t)par[1] + word_to_draw(x, par[0]);
    return x;
  }

  __device__ __forceinline__ int own_pos(int base) const { return base + U * g + q < m ? base + U * g + q : base; }
  __device__ __forceinline__ uint32_t tagged(uint32_t sid) const {
    const uint32_t mb = (meta[sid >> 4] >> (2 * (sid & 15))) & 3u;
    return sid | ((mb & 1u) ? kLongBit : 0u) | ((mb & 2u) ? kYBit : 0u);
  }
  // tickets handed out before the LDS counter exists: two per wavefront (the counter starts behind them)
  static __device__ __forceinline__ int static_tickets() { return 2 * (kLdsBlock / 64) * kTicket; }

  // lane geometry, this wavefront's first two (static) tickets: no memory access
  __device__ __forceinline__ void init(const SagaDev& d, const uint32_t* sp_, int m_, int blk, int nblk,
                                       int* ticket_counter) {
    E = d.cE;                                     // entries in plane P: 12 (response in cmeta) or 11
    in_reg = E + 4;                               // entries of a row held in registers
    y_in_meta = E == 12;
    gl = threadIdx.x & (kLanes8 - 1);
    g = (threadIdx.x & 63) >> 3;                  // group inside the wavefront
    q = gl >> 1;
    is_owner = (gl & 1) == 0;
    in_p = gl < 6;                                // this lane's two entries come from plane P
    slot = in_p ? gl : gl - 6;
    P = d.cP;
    plane = in_p ? d.cP : d.cQ;
    id_off = in_p ? 8 * E + 4 * slot : 8 + 4 * slot;
    v_off = in_p ? 16 * slot : 32 + 16 * slot;
    half = in_p && slot == 5 && E == 11;          // entry 11 of plane P does not exist: the bytes are ids and pad
    sp = sp_;
    meta = d.cmeta;
    m = m_;
    const int share = ((m + nblk - 1) / nblk + kTicket - 1) / kTicket * kTicket;
    tk.counter = ticket_counter;
    tk.lo = blk * share;
    tk.hi = tk.lo + share < m ? tk.lo + share : m;
    tk.m = m;
    tk.dynamic = share >= 4 * (kLdsBlock / 64) * kTicket;
    tk.t = 2;
    const int wave = (int)(threadIdx.x >> 6);
    b_cur = tk.lo + wave * kTicket;
    b_nxt = tk.lo + ((kLdsBlock / 64) + wave) * kTicket;
    if (b_cur >= tk.hi) b_cur = m;
    if (b_nxt >= tk.hi) b_nxt = m;
  }
  // the sample ids of those two tickets (requested, not waited for)
  __device__ __forceinline__ void request_first() {
    s_cur = b_cur < m ? sp[own_pos(b_cur)] : 0u;
    s_nxt = b_nxt < m ? sp[own_pos(b_nxt)] : 0u;
  }
  __device__ __forceinline__ void begin(const SagaDev& d, const uint32_t* sp_, int m_, int blk, int nblk,
                                        int* ticket_counter) {
    init(d, sp_, m_, blk, nblk, ticket_counter);
    request_first();
  }

  __device__ __forceinline__ void tag_first() {
    if (b_cur < m) s_cur = tagged(sample_id(s_cur));
  }

  // all passes of this wavefront; returns the sum of the gradient changes of the draws this lane owns
  __device__ __forceinline__ double run(const SagaDev& d, double b0, const double* wv, double* Dl) {
    double gct = 0.0;
    while (b_cur < m) {
      const bool v_own = b_cur + U * g + q < m;
      uint32_t su[U];
#pragma unroll
      for (int u = 0; u < U; ++u) su[u] = (uint32_t)__shfl((int)s_cur, 2 * u, kLanes8);
      const uint32_t s_this = s_cur & kIdMask;
      double y_own = (s_cur & kYBit) ? 1.0 : 0.0;
      if (!y_in_meta) y_own = *reinterpret_cast<const double*>(P + (size_t)s_this * kCStride + kCYOff);
      int nnz_own = 0;
      if (s_cur & kLongBit) nnz_own = *reinterpret_cast<const int*>(d.cQ + (size_t)s_this * kCStride);
      uint32_t jf[U];
      dpair_t vf[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool on = in_p || (su[u] & kLongBit) != 0;
        const char* base = plane + (size_t)(su[u] & kIdMask) * kCStride;
        jf[u] = 0u;
        vf[u] = dpair_t{0.0, 0.0};
        if (on) {
          jf[u] = *reinterpret_cast<const uint32_t*>(base + id_off);
          vf[u] = *reinterpret_cast<const dpair_t*>(base + v_off);
        }
      }
      // sample ids two passes ahead, their cmeta bits one pass ahead
      const int b_nn = b_nxt < m ? tk.next() : m;
      uint32_t s_nn = 0u;
      if (b_nn < m) s_nn = sp[own_pos(b_nn)];
      if (b_nxt < m) s_nxt = tagged(sample_id(s_nxt));   // (s_nn stays as read: it is in flight)
      if (half) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          vf[u].y = 0.0;
          jf[u] &= 0xffffu;
        }
      }
      double acc[U];
#pragma unroll
      for (int u = 0; u < U; ++u) acc[u] = vf[u].x * wv[jf[u] & 0xffffu] + vf[u].y * wv[jf[u] >> 16];
      const bool own_tail = v_own && nnz_own > in_reg;
      const bool any_tail = __ballot(own_tail) != 0;
      if (any_tail) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int nz = __shfl(own_tail ? nnz_own : 0, 2 * u, kLanes8);
          if (nz > in_reg) {
            double a = 0.0;
            row_tail_compact(d, su[u] & kIdMask, nz, gl, E, [&](int64_t j, double v) { a += v * wv[j]; });
            acc[u] += a;
          }
        }
      }
      const bool hi4 = (gl & 4) != 0, hi2 = (gl & 2) != 0;
      const double r0 = (hi4 ? acc[2] : acc[0]) + __shfl_xor(hi4 ? acc[0] : acc[2], 4, kLanes8);
      const double r1 = (hi4 ? acc[3] : acc[1]) + __shfl_xor(hi4 ? acc[1] : acc[3], 4, kLanes8);
      double t = (hi2 ? r1 : r0) + __shfl_xor(hi2 ? r0 : r1, 2, kLanes8);
      t += __shfl_xor(t, 1, kLanes8);
      const double lp = t + b0;
      const double g0 = d.family == SGDNET_BINOMIAL ? 1.0 - y_own - 1.0 / (1.0 + exp(lp)) : lp - y_own;
      double gcp = 0.0;
      if (is_owner && v_own) {
        // claim, read and update in ONE returning atomic on the line the records came from: a repeated draw of
        // the batch reads back the value just stored (same snapshot, same g0), so its gc is exactly 0
        // (src/saga-sparse.h:281-282)
        const double old = __hip_atomic_exchange(reinterpret_cast<double*>(P + (size_t)s_this * kCStride + kCMOff), g0,
                                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        gcp = g0 - old;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const double gc = __shfl(gcp, 2 * u, kLanes8);
        if (gc != 0.0) {
          if (vf[u].x != 0.0) scatter_add<true>(Dl + (jf[u] & 0xffffu), vf[u].x * gc);
          if (vf[u].y != 0.0) scatter_add<true>(Dl + (jf[u] >> 16), vf[u].y * gc);
          if (any_tail) {
            const int nz = __shfl(own_tail ? nnz_own : 0, 2 * u, kLanes8);
            if (nz > in_reg)
              row_tail_compact(d, su[u] & kIdMask, nz, gl, E,
                               [&](int64_t j, double v) { scatter_add<true>(Dl + j, v * gc); });
          }
        }
      }
      gct += gcp;
      s_cur = s_nxt;
      s_nxt = s_nn;
      b_cur = b_nxt;
      b_nxt = b_nn;
    }
    return gct;
  }
};
typedef K1CompactT<false> K1Compact;

template <int U>
struct K1IdsOnly {
  uint32_t s[U];
  bool valid[U];
  uint32_t s_own;
  bool v_own;
  bool valid_any;
  __device__ __forceinline__ void load(const SagaDev& d, const uint32_t* sp, int i, int hi, int step, int gl,
                                       int safe) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int iu = i + u * step;
      valid[u] = iu < hi;
      s[u] = sp[valid[u] ? iu : safe];
    }
    const int q = U == 4 ? gl >> 2 : gl;
    const int iq = i + q * step;
    v_own = q < U && iq < hi;
    s_own = sp[v_own ? iq : safe];
  }
};

template <int U>
struct K1Draws {
  uint32_t s[U];
  int jf[U], nnz[U];
  double vf[U];
  double gcp;      // on lane owner(u) of the group: gradient change of draw u (0 on the other lanes)
  bool valid[U];
  // this lane's own draw q = draw_of(gl) (its sample and response come from this lane's own loads,
  // not from a selection among the U per-draw registers: such a selection is compiled into an
  // indexed lookup of a private-memory copy of the arrays)
  uint32_t s_own;
  double y_own;
  bool v_own;
  static __device__ __forceinline__ int draw_of(int gl) { return U == 4 ? gl >> 2 : gl; }

  // the lane of the group that evaluates draw u (see gradient())
  static __device__ __forceinline__ int owner(int u) { return U == 4 ? 4 * u : u; }
  static __device__ __forceinline__ bool is_owner(int gl) { return U == 4 ? (gl & 3) == 0 : gl < U; }

  // stream indices + record loads (nothing waits here)
  // `safe` < hi: the draw whose (discarded) record stands in for positions past the end
  __device__ __forceinline__ void load_ids(const SagaDev& d, const uint32_t* sp, int i, int hi, int step, int gl,
                                           int safe) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int iu = i + u * step;
      valid[u] = iu < hi;
      s[u] = sp[valid[u] ? iu : safe];
      if (SGD_ABLATE(d, 16)) s[u] &= 1023u;         // timing only: records from a cache-resident set
    }
    const int q = draw_of(gl);
    const int iq = i + q * step;
    v_own = q < U && iq < hi;
    s_own = sp[v_own ? iq : safe];
    if (SGD_ABLATE(d, 16)) s_own &= 1023u;
  }
  __device__ __forceinline__ void load_records(const SagaDev& d, int gl) {
    const int cap = d.rec_cap;
    y_own = *reinterpret_cast<const double*>(d.rec + (size_t)s_own * d.rec_stride);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const char* base = d.rec + (size_t)s[u] * d.rec_stride;
      nnz[u] = *reinterpret_cast<const int*>(base + 8);
      jf[u] = gl < cap ? reinterpret_cast<const int*>(base + 16)[gl] : 0;
      vf[u] = gl < cap ? reinterpret_cast<const double*>(base + d.rec_val_off)[gl] : 0.0;
    }
  }
  __device__ __forceinline__ void load(const SagaDev& d, const uint32_t* sp, int i, int hi, int step, int gl,
                                       int safe) {
    load_ids(d, sp, i, hi, step, gl, safe);
    load_records(d, gl);
  }
  // the ids of another pass, taken over without touching this pass's records
  template <class O>
  __device__ __forceinline__ void take_ids(const O& o) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      s[u] = o.s[u];
      valid[u] = o.valid[u];
    }
    s_own = o.s_own;
    v_own = o.v_own;
  }
  __device__ __forceinline__ bool in(const SagaDev& d, int u, int gl) const {
    const int cnt0 = nnz[u] < d.rec_cap ? nnz[u] : d.rec_cap;
    return valid[u] && gl < cnt0 && gl < kGroup;
  }
  __device__ __forceinline__ bool tail(const SagaDev& d, int u) const {
    const int cnt0 = nnz[u] < d.rec_cap ? nnz[u] : d.rec_cap;
    return valid[u] && (nnz[u] > cnt0 || cnt0 > kGroup);
  }
  template <class F>
  __device__ __forceinline__ void tail_for_each(const SagaDev& d, int u, int gl, F f) const {
    const char* base = d.rec + (size_t)s[u] * d.rec_stride;
    row_for_each<kGroup, kGroup>(d, base, nnz[u], *reinterpret_cast<const int*>(base + 12), gl, f);
  }
  // x.w, gradient, and the gradient-memory exchange (issued, not waited for)
  __device__ __forceinline__ void gradient(const SagaDev& d, int gl, double b0, const double* wv) {
    double acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = in(d, u, gl) ? vf[u] * (SGD_ABLATE(d, 8) ? 1.0 : wv[jf[u]]) : 0.0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (tail(d, u)) {
        double a = 0.0;
        tail_for_each(d, u, gl, [&](int64_t j, double v) { a += v * wv[j]; });
        acc[u] += a;
      }
    }
    // One gradient evaluation for the U draws of the group.  The exp/division sequence is the
    // bulk of this kernel's vector instructions and costs the same whatever the 64 lanes hold,
    // so the U dot products are reduced TOGETHER: a merged butterfly (U = 4: xor 8 halves four
    // values to two, xor 4 to one, xor 2 and xor 1 finish: 5 shuffles instead of 16) that
    // leaves draw q's x.w in lanes 4q..4q+3 of the group.  Lane owner(q) then evaluates draw
    // q's gradient and issues its exchange: one evaluation and one atomic instruction per U draws.
    double lp_sel = 0.0;
    if (U == 4) {
      const bool hi8 = (gl & 8) != 0, hi4 = (gl & 4) != 0;
      const double r0 = (hi8 ? acc[2] : acc[0]) + __shfl_xor(hi8 ? acc[0] : acc[2], 8, kGroup);
      const double r1 = (hi8 ? acc[3] : acc[1]) + __shfl_xor(hi8 ? acc[1] : acc[3], 8, kGroup);
      double t = (hi4 ? r1 : r0) + __shfl_xor(hi4 ? r0 : r1, 4, kGroup);
      t += __shfl_xor(t, 2, kGroup);
      t += __shfl_xor(t, 1, kGroup);
      lp_sel = t + b0;
    } else {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const double lp = grp_sum<kGroup>(acc[u]) + b0;
        if (gl == owner(u)) lp_sel = lp;
      }
    }
    const double y_sel = y_own;
    const uint32_t s_sel = s_own;
    const bool v_sel = v_own;
    const double g0 = d.family == SGDNET_BINOMIAL ? 1.0 - y_sel - 1.0 / (1.0 + exp(lp_sel)) : lp_sel - y_sel;
    gcp = 0.0;
    if (is_owner(gl) && v_sel) {
      if (SGD_ABLATE(d, 1)) {                        // timing only: no gradient-memory exchange
        gcp = g0;
      } else {
        // claim, read and update in ONE returning atomic: a repeated draw of the batch reads
        // back the value just stored (same snapshot, same g0), so its gc is exactly 0
        const double old = __hip_atomic_exchange(m_slot(d, s_sel), g0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        gcp = g0 - old;
      }
    }
  }
  // LDS scatter of x * gc; returns the sum of gc (lane 0 of the group only)
  __device__ __forceinline__ double scatter(const SagaDev& d, int gl, double* Dl) const {
    double tot = 0.0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const double gc = __shfl(gcp, owner(u), kGroup);
      if (gc != 0.0 && !SGD_ABLATE(d, 4)) {
        if (in(d, u, gl)) scatter_add<true>(Dl + jf[u], vf[u] * gc);
        if (tail(d, u)) tail_for_each(d, u, gl, [&](int64_t j, double v) { scatter_add<true>(Dl + j, v * gc); });
      }
    }
    tot = gcp;     // every draw counted once: on its owner lane
    return tot;
  }
};

}  // namespace sgdnet
