// The multinomial Newton modes under the GROUPED penalty (type_multinomial = 1 with the option "mnewton_grouped" = 1): the
// inner solves and the publish that mnewton.hip's outer loop launches in place of mnewton_cd_kernel, mnewton_wide_cd_kernel
// and the blend kernels.  Everything else of a step -- the state pass, the class-pair moments, mnewton_wide_scale_kernel,
// the line search -- does not depend on the penalty and is mnewton.hip's, unchanged.
//
// The model of one outer step about the iterate U0, over the Q = K P coordinates (k, j) at k P + j, P = p + 1, j = p the
// intercept (mnewton.hip):
//     (U - U0)'H (U - U0) / 2 - q'(U - U0) + sum_j (al/2 |w_.j|^2 + be |w_.j|_2),      g = H (U - U0) - q its smooth gradient,
// w_.j the K coefficients of feature j: BLOCK j, the coordinates k P + j.  The penalty does not separate over the
// coordinates of a block, so the blocks move whole, by a majorised proximal step (block coordinate gradient descent, Tseng
// & Yun 2009): with t_j = max_k sum_l |H[(k, j), (l, j)]| -- Gershgorin's bound of the block's K x K Hessian, at least its
// largest eigenvalue -- the model along the block lies below its value at u_j plus g_j'd + t_j |d|^2 / 2, whose penalised
// minimiser is
//     z = t_j u_j - g_j,      v = z max(0, 1 - be / |z|_2) / (t_j + al).
// v = u_j exactly where u_j satisfies the block's optimality conditions (g_j + al u_j + be u_j / |u_j| = 0, or |g_j| <= be
// at u_j = 0), so the fixed points of a sweep are the KKT points of the model and the outer loop ends at the grouped
// optimum.  t_j = 0 without an l2 term: the block stays (a constant column: its rows of H and its q are 0).  What the
// threshold leaves of a block when |z| equals it but for rounding is an exact zero: t_j |v|^2 <= kNewtonNegligible^2
// (newton.hpp) gives v = 0, the block form of mnewton_cd_kernel's rule.  The K intercepts are scalar unpenalised
// coordinates, updated as mnewton_cd_kernel updates them; a frozen intercept is never visited.  A sweep visits the blocks
// j = 0 .. p - 1, then the intercepts k = 0 .. K - 1.  No exact K x K block solve is attempted.
//
// Every lane computes a block's scalars -- |z|^2 summed over k = 0 .. K - 1 in that order, the factor, the sweep's maxima
// -- from the same LDS words, so the branches on them are uniform and nothing is broadcast.  A block that moves stores its
// K steps d_k to LDS (lane k), and g is updated in ONE pass, g[c] += sum_k H[c, (k, j)] d_k with k ascending, an entry (wide:
// 16 bytes) per lane: one barrier pair per block, not K, and the same bits whatever the workgroup's width.
//
// The record: kRecAbs holds sum_j |w_.j|_2, so that the host's objective loss + al kRecHalfSq + be kRecAbs is the grouped
// one and the line search weighs it; everything else as mnewton_publish writes it.  The stopping quantities of a sweep are
// max|d| (a block's scaled: grouped_change_scale), max|v| and max t_j |v_.j|^2 (intercepts: H_cc v^2) in mnewton_cd_kernel's slots.
//
// No floating-point atomic, every reduction in an order fixed by (p, K): the same input gives the same bits.
#define SGDNET_DET_MATH
#include "mnewton_grouped.hpp"

#include "common.hpp"
#include "device_math.hpp"
#include "mnewton.hpp"
#include "moments_device.hpp"
#include "newton_cv_device.hpp"
#include "wide_cd_device.hpp"

namespace sgdnet {
namespace {

// (mnewton.hip: the class pair (k <= l) of the moments M)
__device__ __forceinline__ int class_pair_index(int k, int l, int K) { return k * K - k * (k - 1) / 2 + (l - k); }

// The factor f of a block's step v_k = f z_k, z_k = t u_k - g_k, from the block's words u[k P], g[k P] (k = 0 .. K - 1) in
// LDS; *stays: t + al is not positive and the block keeps its values.  *eta_sq = t |v|^2, the block's "size to rounding".
__device__ __forceinline__ double grouped_block_factor(double t, const double* ub, const double* gb, int P, int K, double al, double be,
                                                       bool* stays, double* eta_sq) {
  const double denom = t + al;
  *stays = !(denom > 0.0);
  *eta_sq = 0.0;
  if (*stays) return 0.0;
  double nz2 = 0.0;
  for (int k = 0; k < K; ++k) {
    const double z = t * ub[k * P] - gb[k * P];
    nz2 += z * z;
  }
  const double nz = sqrt(nz2);
  double f = nz > be ? (1.0 - be / nz) / denom : 0.0;
  double e = t * (f * f * nz2);
  if (e <= kNewtonNegligible * kNewtonNegligible) {         // zero to rounding: an exact zero (see above)
    f = 0.0;
    e = 0.0;
  }
  *eta_sq = e;
  return f;
}

// What a sweep counts a block's step d as: |d| (t + al) / (hmin + al), hmin the smallest of the block's K diagonal entries
// of H -- about the step an exact coordinate update would have taken from the same gradient, since the majorised step
// divides by t + al where that one divides by H_cc + al.  Without it a sweep of short majorised steps met the relative-change
// test while the model was further from its optimum than mnewton_cd_kernel leaves it: at the default thresh the grouped
// fits' worst KKT ratio was 3.4 x the ungrouped modes' (0.143 against 0.042, profiles/mnewton_grouped.txt).
__device__ __forceinline__ double grouped_change_scale(double t, double hmin, double al) {
  return hmin + al > 0.0 ? (t + al) / (hmin + al) : 1.0;
}

// mnewton_publish under the grouped penalty, by the workgroup's first wavefront, from the candidate un[0 .. Q) in LDS: lane
// l takes the coordinates l, l + 64, ... for the candidate's two forms, sum w^2 / 2, the change and the size, then the
// features l, l + 64, ... with their classes in order for sum_j |w_.j|_2; the lanes are joined by a butterfly.
__device__ __forceinline__ void grouped_publish(const double* un, const double* __restrict__ u_cur, const double* __restrict__ scale, int p,
                                                int K, double* __restrict__ u_cand, double* __restrict__ a_cand, double* __restrict__ rec) {
  const int lane = threadIdx.x, P = p + 1, Q = K * P;
  if (lane >= 64) return;
  double sq = 0.0, ab = 0.0, ch = 0.0, sz = 0.0;
  for (int c = lane; c < Q; c += 64) {
    const int j = c % P;
    const double uc = un[c];
    ch = fmax(ch, fabs(uc - u_cur[c]));
    sz = fmax(sz, fabs(uc));
    if (j < p) sq += uc * uc;
    u_cand[c] = uc;
    a_cand[c] = j < p ? uc / scale[j] : uc;
  }
  for (int j = lane; j < p; j += 64) {
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += un[k * P + j] * un[k * P + j];
    ab += sqrt(s);
  }
  sq = wave_sum(sq);
  ab = wave_sum(ab);
  ch = wave_max(ch);
  sz = wave_max(sz);
  if (lane == 0) {
    rec[kRecHalfSq] = 0.5 * sq;
    rec[kRecAbs] = ab;
    rec[kRecChange] = ch;
    rec[kRecSize] = sz;
  }
}

// u_cand <- u_cur + t (u_cand - u_cur) (t = 1: as it is), published with the grouped record.  kCap: the mode's most
// coordinates; the candidate is formed in LDS before any of it is overwritten.
template <int kCap>
__global__ __launch_bounds__(64) void mnewton_grouped_blend_kernel(const double* __restrict__ u_cur, const double* __restrict__ scale, int p,
                                                                    int K, double t, double* u_cand, double* __restrict__ a_cand,
                                                                    double* __restrict__ rec) {
  __shared__ double un[kCap];
  const int Q = K * (p + 1);
  for (int c = threadIdx.x; c < Q; c += 64) un[c] = t == 1.0 ? u_cand[c] : u_cur[c] + t * (u_cand[c] - u_cur[c]);
  __syncthreads();
  grouped_publish(un, u_cur, scale, p, K, u_cand, a_cand, rec);
}

// The narrow inner solve: one workgroup of kWidth lanes (64 or 256).  LDS: mnewton_cd_kernel's packed triangle, U and g, with
// that kernel's prologue (the same bits), then T[0 .. p) = t_j and S[0 .. p) = the blocks' change scales, computed once per
// solve with the lanes spread over j, and d[0 .. K), the steps of the block that moves (mnewton.hpp:
// mnewton_grouped_state_doubles).
template <int kWidth>
__global__ __launch_bounds__(kWidth) void mnewton_grouped_cd_kernel(const double* __restrict__ M, const double* __restrict__ scale, int p, int K,
                                                                     double dn, const double* __restrict__ u_cur, double al, double be,
                                                                     int fit_intercept, unsigned max_sweeps, double tol,
                                                                     double* __restrict__ u_cand, double* __restrict__ a_cand,
                                                                     double* __restrict__ rec) {
  // (the whole 160 KiB, where mnewton_cd_kernel declares mnewton_state_doubles(199): T, S and d lie behind its layout.  The
  // prologue below is mnewton_cd_solve's text: an edit there is an edit here, or the two stop holding the same H, g and U.)
  __shared__ double lds[kNewtonLdsDoubles];
  constexpr int kOwn = (kWmnewtonMaxClasses + kWidth - 1) / kWidth;        // the classes k = lane, lane + kWidth, ... of a lane
  const int lane = threadIdx.x, P = p + 1, nc = p + 2, Q = K * P;
  const size_t block = (size_t)nc * (size_t)nc;
  double* H = lds;
  double* u = H + Q * (Q + 1) / 2;
  double* g = u + Q;
  double* T = g + Q;
  double* S = T + p;
  double* dblk = S + p;
  for (int c2 = 0; c2 < Q; ++c2) {
    const int l = c2 / P, b = c2 - l * P;
    const double sb = b < p ? scale[b] : 1.0;
    for (int c1 = lane; c1 <= c2; c1 += kWidth) {
      const int k = c1 / P, a = c1 - k * P;         // k <= l
      const int lo = a < b ? a : b, hi = a < b ? b : a;
      H[tri(c1, c2)] = M[(size_t)class_pair_index(k, l, K) * block + (size_t)lo * nc + hi] / dn / ((a < p ? scale[a] : 1.0) * sb);
    }
  }
  for (int c = lane; c < Q; c += kWidth) {
    const int k = c / P, a = c - k * P;
    g[c] = -(M[(size_t)class_pair_index(k, k, K) * block + (size_t)a * nc + p + 1] / dn / (a < p ? scale[a] : 1.0));
    u[c] = u_cur[c];
  }
  __syncthreads();
  for (int j = lane; j < p; j += kWidth) {
    double t = 0.0, hmin = 0.0;
    for (int k = 0; k < K; ++k) {
      double s = 0.0;
      for (int l = 0; l < K; ++l) {
        const int c1 = k * P + j, c2 = l * P + j;
        s += fabs(H[c1 <= c2 ? tri(c1, c2) : tri(c2, c1)]);
      }
      t = fmax(t, s);
      const double hkk = H[tri(k * P + j, k * P + j)];
      hmin = k == 0 ? hkk : fmin(hmin, hkk);
    }
    T[j] = t;
    S[j] = grouped_change_scale(t, hmin, al);
  }
  __syncthreads();
  unsigned sweeps = 0;
  bool converged = false, negligible = false;
  while (sweeps < max_sweeps && !converged) {
    double max_change = 0.0, max_size = 0.0, max_eta_sq = 0.0;
    for (int j = 0; j < p; ++j) {
      const double t = T[j];
      bool stays;
      double eta_sq;
      const double f = grouped_block_factor(t, u + j, g + j, P, K, al, be, &stays, &eta_sq);
      bool moved = false;
      for (int k = 0; k < K; ++k) {
        const double uk = u[k * P + j], v = stays ? uk : (t * uk - g[k * P + j]) * f, d = v - uk;
        max_change = fmax(max_change, fabs(d) * S[j]);
        max_size = fmax(max_size, fabs(v));
        moved |= d != 0.0;
      }
      max_eta_sq = fmax(max_eta_sq, eta_sq);
      if (moved) {
        double v_own[kOwn];
#pragma unroll
        for (int i = 0; i < kOwn; ++i) {
          const int k = lane + i * kWidth;
          v_own[i] = 0.0;
          if (k < K) {
            const double uk = u[k * P + j];
            v_own[i] = (t * uk - g[k * P + j]) * f;
            dblk[k] = v_own[i] - uk;
          }
        }
        __syncthreads();                           // every lane has read the block's u and g; d is there
#pragma unroll
        for (int i = 0; i < kOwn; ++i) {
          const int k = lane + i * kWidth;
          if (k < K) u[k * P + j] = v_own[i];
        }
        for (int c = lane; c < Q; c += kWidth) {
          double acc = g[c];
          for (int k = 0; k < K; ++k) {
            const int cj = k * P + j;
            acc += H[c <= cj ? tri(c, cj) : tri(cj, c)] * dblk[k];
          }
          g[c] = acc;
        }
        __syncthreads();
      }
    }
    if (fit_intercept)                             // (the frozen intercepts are never visited: they stay at u_cur)
      for (int k = 0; k < K; ++k) {
        const int j = k * P + p;
        const double uj = u[j], hjj = H[tri(j, j)];
        const double nu = hjj > 0.0 ? (hjj * uj - g[j]) / hjj : uj;      // every weight underflowed: the coordinate stays
        const double d = nu - uj;
        max_change = fmax(max_change, fabs(d));
        max_size = fmax(max_size, fabs(nu));
        max_eta_sq = fmax(max_eta_sq, nu * nu * hjj);
        if (d != 0.0) {
          __syncthreads();                         // every lane has read u[j] and g[j]
          if (lane == 0) u[j] = nu;
          for (int c = lane; c < Q; c += kWidth) g[c] += H[c <= j ? tri(c, j) : tri(j, c)] * d;
          __syncthreads();
        }
      }
    ++sweeps;
    const bool all_zero = max_size == 0.0 && max_change == 0.0;
    const bool no_change = max_size != 0.0 && max_change / max_size <= tol;
    negligible = max_eta_sq <= kNewtonNegligible * kNewtonNegligible;      // zero to rounding (newton.hpp)
    converged = all_zero || no_change || negligible;
  }
  __syncthreads();
  grouped_publish(u, u_cur, scale, p, K, u_cand, a_cand, rec);
  if (lane == 0) {
    rec[kRecSweeps] = (double)sweeps;
    rec[kRecInnerConverged] = converged ? 1.0 : 0.0;
    rec[kRecNegligible] = negligible ? 1.0 : 0.0;
  }
}

// g[c] += sum_k H[c, k P + j] d[k] for all c < Q, k ascending: a lane owns the slots s = lane, lane + kWidth, ...; a slot is
// c = 2 s and 2 s + 1, 16 bytes of each of the block's K columns, accumulated in registers before the one store to g
// (wide_column_move's slots; Q odd: the last one's second entry is H's zero pad, and g's is not touched).
template <int kWidth>
__device__ __forceinline__ void wide_block_move(double* g, const double* __restrict__ H, int ld, int j, int P, int K, int Q,
                                                const double* dblk) {
  const int slots = (Q + 1) / 2;
  for (int s = threadIdx.x; s < slots; s += kWidth) {
    const int c = 2 * s;
    const bool two = c + 1 < Q;
    double a0 = g[c], a1 = two ? g[c + 1] : 0.0;
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
      const double2 v = *reinterpret_cast<const double2*>(H + (size_t)ld * (size_t)(k * P + j) + c);
      const double d = dblk[k];
      a0 = fma(v.x, d, a0);
      a1 = fma(v.y, d, a1);
    }
    g[c] = a0;
    if (two) g[c + 1] = a1;
  }
}

// The wide inner solve: one workgroup of kWidth lanes (256 or 1024), H (leading dimension ld, a multiple of 16), diag H and
// q as mnewton_wide_scale_kernel wrote them.  The ENTRIES of the list are the blocks e = j < p and the intercepts e = p + k,
// E = p + K of them.  LDS (mnewton.hpp: wmnewton_grouped_state_bytes): g | U | T | S | d | the list | its bits | the counts,
// with T[j] = t_j, read once per solve from the block's K x K entries in global memory (the lanes spread over j),
// T[p + k] = H's diagonal at the intercept of class k, and S[j] the blocks' change scales.
//   start    U = U_cur, g = -q.  The list: the blocks with a coordinate != 0, and the intercepts when they are fitted.
//   screen   a block outside the list (all its coordinates are 0) joins iff its step from 0 is not 0: |g_.j|_2 > be and
//            what is left is not zero to rounding.  Ascending again (wide_compact).
//   sweep    the block step over the list; a block that stays costs no global read and no barrier; one that moves reads
//            its K columns in one fused pass over all c < Q (wide_block_move), so g stays the full gradient.  The sweeps and
//            the screens end as mnewton_wide_cd_kernel's do.
template <int kWidth>
__global__ __launch_bounds__(kWidth) void mnewton_wide_grouped_cd_kernel(const double* __restrict__ H, const double* __restrict__ Hd,
                                                                          const double* __restrict__ q, const double* __restrict__ scale, int p,
                                                                          int K, int ld, const double* __restrict__ u_cur, double al, double be,
                                                                          int fit_intercept, unsigned max_sweeps, double tol,
                                                                          double* __restrict__ u_cand, double* __restrict__ a_cand,
                                                                          double* __restrict__ rec) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[kWmnewtonLdsBytes];
  static_assert(kWidth >= kWmnewtonMaxClasses, "lane k owns class k of the block that moves");
  const int lane = threadIdx.x, wave = lane >> 6, P = p + 1, Q = K * P, E = p + K;
  double* g = reinterpret_cast<double*>(lds);
  double* u = g + Q;
  double* T = u + Q;
  double* S = T + E;
  double* dblk = S + p;
  int32_t* list = reinterpret_cast<int32_t*>(dblk + K);
  uint32_t* bits = reinterpret_cast<uint32_t*>(list + E);
  int32_t* counts = reinterpret_cast<int32_t*>(bits + (E + 31) / 32);
  for (int c = lane; c < Q; c += kWidth) {
    g[c] = -q[c];
    u[c] = u_cur[c];
  }
  for (int e = lane; e < E; e += kWidth) {
    double t = 0.0;
    if (e < p) {
      double hmin = 0.0;
      for (int k = 0; k < K; ++k) {
        double s = 0.0;
        for (int l = 0; l < K; ++l) s += fabs(H[(size_t)ld * (size_t)(l * P + e) + (size_t)(k * P + e)]);
        t = fmax(t, s);
        const double hkk = Hd[k * P + e];
        hmin = k == 0 ? hkk : fmin(hmin, hkk);
      }
      S[e] = grouped_change_scale(t, hmin, al);
    } else {
      t = Hd[(e - p) * P + p];
    }
    T[e] = t;
  }
  __syncthreads();

  // The list from one flag per entry (wide_compact).  screen: "in the list already, or would move from 0"; else: the start's.
  auto compact = [&](bool screen) -> int {
    return wide_compact<kWidth>(E, list, bits, counts, [&](int e) -> bool {
      bool in = false;
      if (e < p) {
        if (screen) {
          in = (bits[e >> 5] >> (e & 31)) & 1u;
          if (!in) {
            bool stays;
            double eta_sq;
            in = grouped_block_factor(T[e], u + e, g + e, P, K, al, be, &stays, &eta_sq) != 0.0;
          }
        } else {
          for (int k = 0; k < K; ++k) in |= u[k * P + e] != 0.0;
        }
      } else if (e < E) {
        in = fit_intercept != 0;
      }
      return in;
    });
  };

  int n_list = compact(false);
  unsigned sweeps = 0;
  bool converged = false, negligible = false;
  for (int screens = 0;; ++screens) {
    const int n_new = compact(true);
    if (screens > 0 && n_new == n_list) {        // the list had converged and nothing outside it moves
      converged = true;
      break;
    }
    n_list = n_new;
    bool met = false;
    while (sweeps < max_sweeps && !met) {
      double max_change = 0.0, max_size = 0.0, max_eta_sq = 0.0;
      for (int i = 0; i < n_list; ++i) {
        const int e = list[i];
        const double t = T[e];
        if (e < p) {
          bool stays;
          double eta_sq;
          const double f = grouped_block_factor(t, u + e, g + e, P, K, al, be, &stays, &eta_sq);
          bool moved = false;
          for (int k = 0; k < K; ++k) {
            const double uk = u[k * P + e], v = stays ? uk : (t * uk - g[k * P + e]) * f, d = v - uk;
            max_change = fmax(max_change, fabs(d) * S[e]);
            max_size = fmax(max_size, fabs(v));
            moved |= d != 0.0;
          }
          max_eta_sq = fmax(max_eta_sq, eta_sq);
          if (moved) {
            double v_own = 0.0;
            if (lane < K) {
              const double uk = u[lane * P + e];
              v_own = (t * uk - g[lane * P + e]) * f;
              dblk[lane] = v_own - uk;
            }
            __syncthreads();                       // every lane has read the block's u and g; d is there
            if (lane < K) u[lane * P + e] = v_own;
            wide_block_move<kWidth>(g, H, ld, e, P, K, Q, dblk);
            __syncthreads();
          }
        } else {
          const int c = (e - p) * P + p;
          const double uj = u[c];
          const double nu = t > 0.0 ? (t * uj - g[c]) / t : uj;
          const double d = nu - uj;
          max_change = fmax(max_change, fabs(d));
          max_size = fmax(max_size, fabs(nu));
          max_eta_sq = fmax(max_eta_sq, nu * nu * t);
          if (d != 0.0) {
            __syncthreads();                       // every lane has read u[c] and g[c]
            if (lane == 0) u[c] = nu;
            wide_column_move<kWidth>(g, H + (size_t)ld * c, Q, d);
            __syncthreads();
          }
        }
      }
      ++sweeps;
      const bool all_zero = max_size == 0.0 && max_change == 0.0;
      const bool no_change = max_size != 0.0 && max_change / max_size <= tol;
      negligible = max_eta_sq <= kNewtonNegligible * kNewtonNegligible;      // zero to rounding (newton.hpp)
      met = all_zero || no_change || negligible;
    }
    if (!met) break;                               // max_sweeps: the next outer step goes on from here
  }
  __syncthreads();
  if (wave == 0) {
    grouped_publish(u, u_cur, scale, p, K, u_cand, a_cand, rec);
    if (lane == 0) {
      rec[kRecSweeps] = (double)sweeps;
      rec[kRecInnerConverged] = converged ? 1.0 : 0.0;
      rec[kRecNegligible] = negligible ? 1.0 : 0.0;
    }
  }
}

}  // namespace

void mnewton_grouped_cd(int width, const double* M, const double* scale, int p, int K, double dn, const double* u_cur, double al, double be,
                        int fit_intercept, unsigned max_sweeps, double tol, double* u_cand, double* a_cand, double* rec, hipStream_t st) {
  const auto kernel = width == 256 ? mnewton_grouped_cd_kernel<256> : mnewton_grouped_cd_kernel<64>;
  hipLaunchKernelGGL(kernel, dim3(1), dim3(width == 256 ? 256u : 64u), 0, st, M, scale, p, K, dn, u_cur, al, be, fit_intercept, max_sweeps, tol,
                     u_cand, a_cand, rec);
}

void mnewton_wide_grouped_cd(int width, const double* H, const double* Hd, const double* q, const double* scale, int p, int K, int ld,
                             const double* u_cur, double al, double be, int fit_intercept, unsigned max_sweeps, double tol, double* u_cand,
                             double* a_cand, double* rec, hipStream_t st) {
  const auto kernel = width == kWideNarrow ? mnewton_wide_grouped_cd_kernel<kWideNarrow> : mnewton_wide_grouped_cd_kernel<kWideFull>;
  hipLaunchKernelGGL(kernel, dim3(1), dim3(width == kWideNarrow ? (unsigned)kWideNarrow : (unsigned)kWideFull), 0, st, H, Hd, q, scale, p, K, ld,
                     u_cur, al, be, fit_intercept, max_sweeps, tol, u_cand, a_cand, rec);
}

void mnewton_grouped_blend(bool wide, const double* u_cur, const double* scale, int p, int Q, double t, double* u_cand, double* a_cand,
                           double* rec, hipStream_t st) {
  const int K = Q / (p + 1);
  if (wide)
    hipLaunchKernelGGL(mnewton_grouped_blend_kernel<kWmnewtonMaxCoordinates>, dim3(1), dim3(64), 0, st, u_cur, scale, p, K, t, u_cand, a_cand, rec);
  else
    hipLaunchKernelGGL(mnewton_grouped_blend_kernel<kMNewtonMaxCoordinates>, dim3(1), dim3(64), 0, st, u_cur, scale, p, K, t, u_cand, a_cand, rec);
}

}  // namespace sgdnet
