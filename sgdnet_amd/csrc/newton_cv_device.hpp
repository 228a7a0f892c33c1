// What the lock-step cross-validations of the Newton modes share (newton.hip: newton_cv_run, mnewton.hip: mnewton_cv_run):
// the record of a candidate, the command and the geometry of a job as the kernels read them, and the host's state
// machine of one job between two rounds.  Included by those two files only (HIP types in here).
#pragma once

#include <math.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "newton.hpp"

namespace sgdnet {

// the record of a candidate, in device memory; the host reads it after every state pass
enum Rec { kRecLoss = 0, kRecHalfSq, kRecAbs, kRecChange, kRecSize, kRecSweeps, kRecInnerConverged, kRecNegligible, kRecLen };

// A job is one (mix, training set).  x and y hold the rows sorted by group, so the rows of a training set are one range
// of rows or two: [a0, a1) and [b0, b1) (the second empty when the job trains on its own group).  Row li of the job's
// problem, li = 0 .. n_t - 1, is row cv_row(J, li) of x; a job visits its own rows only.  The host sends one CvCmd per
// job and round.
enum CvAction { kCvIdle = 0, kCvStep, kCvHalve, kCvStart };

struct CvCmd {
  int32_t action;          // CvAction; kCvStart: publish the path's start and evaluate it
  int32_t cur;             // which of the job's two iterates is the current one (the other holds the candidate)
  int32_t slot;            // >= 0: the current iterate is the answer for this lambda: store it into U[slot] first
  int32_t ridge;
  double l2, l1;           // this lambda's penalties
};

struct CvJob {
  int64_t a0, a1, b0, b1;  // the rows of the training set
  int64_t n_t;
  int64_t rows_per_chunk;  // dense x: dense_rows_per_chunk(n_t, the workgroups of a chunk)
  int32_t set;             // the training set: whose centres and scales
  int32_t state_blocks, chunks, pad;
};

__device__ __forceinline__ int64_t cv_row(const CvJob& J, int64_t li) {
  const int64_t la = J.a1 - J.a0;
  return li < la ? J.a0 + li : J.b0 + (li - la);
}

// the rows of training set t of `job`: group t, [start[t], start[t + 1]), or everything else
inline void cv_job_rows(CvJob& J, const int64_t* start, int64_t n, bool train_on_rest) {
  const int t = J.set;
  if (train_on_rest) {
    J.a0 = 0;
    J.a1 = start[t];
    J.b0 = start[t + 1];
    J.b1 = n;
  } else {
    J.a0 = start[t];
    J.a1 = J.b0 = J.b1 = start[t + 1];
  }
}

// what the host knows of a job between two rounds: the local variables of newton_run / mnewton_run
struct CvJobState {
  int l = 0, cur = 0, halved = 0, action = kCvStart, slot = -1;
  unsigned steps = 0;
  bool negligible = false;
  double objective = 0.0, candidate = 0.0, loss = 0.0, half_sq = 0.0, abs1 = 0.0;
};

struct CvPinned {
  void* p = nullptr;
  ~CvPinned() {
    if (p) (void)hipHostFree(p);
  }
};

// the command of a round from the job's state; penalties(l, &al, &be): the job's penalties at lambda l, read by a step only
template <class Penalties>
inline void cv_command(CvCmd& c, const CvJobState& s, bool ridge, Penalties&& penalties) {
  c.action = s.action;
  c.cur = s.cur;
  c.slot = s.slot;
  c.ridge = ridge ? 1 : 0;
  c.l2 = c.l1 = 0.0;
  if (s.action == kCvStep) penalties(s.l, &c.l2, &c.l1);
}

// What a round's record means for one job: its state machine moves exactly as newton_run moves its one.  A step is
// (moments, inner solve, state pass at the candidate); a candidate after which the objective rose is halved (blend, state
// pass) in the next round; an accepted candidate becomes the current iterate by flipping `cur`; a lambda that is done names
// the slot of U its iterate goes to.  penalties(l, &al, &be): the job's penalties at lambda l.  loss, unconverged: the
// job's n_lambda entries; passes, steps, halvings: the job's counters; sweeps: the call's.  True: the job has finished
// its last lambda in this round.
template <class Penalties>
inline bool cv_job_advance(CvJobState& s, const double* rec, int n_lambda, unsigned max_iter, double tol, Penalties&& penalties,
                           double* loss, int32_t* unconverged, double* passes, double* steps, double* halvings, double* sweeps) {
  const int did = s.action;
  s.slot = -1;
  if (did == kCvIdle) return false;
  *passes += 1.0;
  double al, be;
  penalties(s.l, &al, &be);
  if (did == kCvStart) {           // the path's start: w = 0, b = b0
    s.loss = rec[kRecLoss];
    s.half_sq = rec[kRecHalfSq];
    s.abs1 = rec[kRecAbs];
    s.objective = s.loss + al * s.half_sq + be * s.abs1;
    s.steps = 0;
    s.action = kCvStep;
    return false;
  }
  if (did == kCvStep) {
    *sweeps += rec[kRecSweeps];
    s.negligible = rec[kRecNegligible] != 0.0;
    s.halved = 0;
  } else {
    *halvings += 1.0;
    s.negligible = false;          // (the inner solve said so of the whole step, not of a part of it)
  }
  s.candidate = rec[kRecLoss] + al * rec[kRecHalfSq] + be * rec[kRecAbs];
  // (a candidate whose objective is not a number counts as one that rose)
  if (s.halved < kNewtonMaxHalvings && rec[kRecChange] > 0.0 && !(s.candidate <= s.objective + kNewtonObjectiveSlack * fabs(s.objective))) {
    ++s.halved;
    s.action = kCvHalve;
    return false;
  }
  s.cur ^= 1;                      // accepted: the candidate is the iterate
  s.objective = s.candidate;
  s.loss = rec[kRecLoss];
  s.half_sq = rec[kRecHalfSq];
  s.abs1 = rec[kRecAbs];
  ++s.steps;
  *steps += 1.0;
  const double change = rec[kRecChange], size = rec[kRecSize];
  const bool all_zero = size == 0.0 && change == 0.0;
  const bool no_change = size != 0.0 && change / size <= tol;
  const bool converged = rec[kRecInnerConverged] != 0.0 && (all_zero || no_change || s.negligible);
  s.action = kCvStep;
  if (!converged && s.steps < max_iter) return false;
  loss[s.l] = s.loss;
  unconverged[s.l] = converged ? 0 : 1;
  s.slot = s.l++;
  s.steps = 0;
  if (s.l == n_lambda) {
    s.action = kCvIdle;
    return true;
  }
  penalties(s.l, &al, &be);
  s.objective = s.loss + al * s.half_sq + be * s.abs1;
  return false;
}

}  // namespace sgdnet
