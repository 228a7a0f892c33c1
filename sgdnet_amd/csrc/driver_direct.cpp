// The direct modes behind sgdnet_fit_* / sgdnet_cv_* (fit_plan.hpp: is_direct_mode): the path comes from a Gram or Hessian
// matrix on the device (covariance.hip, newton.hip, mnewton.hip), no SAGA solver is created and no sample is drawn.
//
//   fit_direct          the stage behind the plan (driver.cpp: fit_common calls it once plan_fit accepted the fit): the
//                       problem every mode fills the same way, the kernels' run, and per lambda the deviance and the way
//                       back to the scale of the data
//   fit_cv_covariance   every fold fit of a cross-validation in one launch       (sgdnet_cv_covariance_*, sgdnet_cv_wcovariance_*)
//   fit_cv_mcovariance  the same for the K responses of an mgaussian fit         (sgdnet_cv_mcovariance_*, sgdnet_cv_wmcovariance_*)
//   fit_cv_newton       every fold fit through the Newton loop in lock-step      (sgdnet_cv_newton_*)
//   fit_cv_mnewton      the same through the multinomial Newton loop             (sgdnet_cv_mnewton_*)
//   the probes          one outer step of the Newton modes, everything copied back (sgdnet_newton_probe_*, sgdnet_mnewton_probe)
#include <math.h>

#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

#include "driver_parts.hpp"

using namespace sgdnet;

namespace {

// ---- the stages behind the plan ----
// The preprocessed problem is the one every mode fits: features (x_j - x_center_j) / x_scale_j (x_center = 0, x_scale = 1
// without standardize), the response of prepare_response, the penalties of regularization_path.  With an intercept the
// optimum only sees deviations from the column means, standardised or not; without one the intercept stays at the null
// model's value and the features are taken as the preprocessing left them: deviations from x_center.

// what every direct problem takes from the features, the path, the plan and the control
void fill_problem(DirectProblem& pb, const Features& X, const Path& path, const FitPlan& plan, const sgdnet_control* ctl) {
  pb.n = X.n;
  pb.p = X.p;
  if (X.sparse) {
    pb.colptr = X.colptr;
    pb.rowidx = X.rowidx;
    pb.values = X.raw_values;
  } else {
    pb.x_dense = X.raw_dense;
  }
  pb.centre = ctl->intercept != 0 || ctl->standardize != 0;
  pb.scale = X.x_scale.data();
  pb.device = plan.rank_dev[0];
  pb.n_lambda = ctl->n_lambda;
  pb.alpha = path.alpha.data();
  pb.beta = path.beta.data();
  pb.ridge = plan.penalty == SGDNET_RIDGE;
  pb.max_iter = ctl->max_iter;
  pb.tol = ctl->tol;
}

// The intercepts of the preprocessed problem, b (K).  The kernels took deviations from `mean` (p), the preprocessing from
// x_center: a fitted intercept is the one at the kernels' centres, at_centres (K), less the centres' distance from
// x_center times w (K x p, entry (k, j) at k + j K); one that is not fitted stays at the null model's value.
void intercepts_at_x_center(const Features& X, const Response& R, const sgdnet_control* ctl, const double* mean, const double* w,
                            const double* at_centres, double* b) {
  const int K = ctl->n_classes;
  for (int k = 0; k < K; ++k) {
    double shift = 0.0;
    for (int64_t j = 0; j < X.p; ++j) shift += (mean[j] - X.x_center[(size_t)j]) / X.x_scale[(size_t)j] * w[k + j * K];
    b[k] = ctl->intercept != 0 ? at_centres[k] - shift : R.b0[(size_t)k];
  }
}

// lambda li is done: what every mode returns of it besides its deviance
void lambda_done(const Features& X, const Response& R, const Path& path, const sgdnet_control* ctl, int li, bool unconverged,
                 const double* w, const double* b, sgdnet_result* out) {
  out->lambda[li] = path.lambda[(size_t)li];
  out->return_codes[li] = unconverged ? 1.0 : 0.0;
  rescale_values(X, R, ctl, li, w, b, out);
}

// ---- covariance mode (SGDNET_MODE_COVARIANCE, covariance.hip) ----
// SGDNET_MODE_WCOVARIANCE is the same stage around wcovariance_run (S in global memory, any p up to its own limit).
int fit_covariance(const Features& X, const Response& R, const Path& path, const FitPlan& plan, const sgdnet_control* ctl,
                   sgdnet_result* out, PhaseTimer& pt) {
  const bool wide = plan.mode == SGDNET_MODE_WCOVARIANCE;
  const int64_t n = X.n, p = X.p;
  const int L = ctl->n_lambda;
  CovarianceProblem pb;
  fill_problem(pb, X, path, plan, ctl);
  pb.y = R.y.data();
  CovarianceResult cr;
  int rc = wide ? wcovariance_run(pb, &cr, option(kOptWcovarianceWidth)) : covariance_run(pb, &cr);
  if (rc) return rc;
  if (pt.on && wide)
    fprintf(stderr, "[sgdnet]   wcovariance: moments %.3f ms, scale %.3f ms, path kernel %.3f ms\n", cr.moments_ms, cr.scale_ms, cr.path_ms);
  else if (pt.on)
    fprintf(stderr, "[sgdnet]   covariance: moments %.3f ms, path kernel %.3f ms\n", cr.moments_ms, cr.path_ms);

  // deviance from the quadratic form: |y~ - X~ w|^2 = y~'y~ - n (2 c~'w - w'S w), and w'S w = w'(g + c~) with the path
  // kernel's gradient g = S w - c~: the explained part is n sum_j w_j (c~_j - g_j), each term w_j c~_j + alpha w_j^2 +
  // beta |w_j| at the optimum
  double yy = 0.0;
  for (int64_t i = 0; i < n; ++i) yy += R.y[(size_t)i] * R.y[(size_t)i];
  double n_sweeps = 0.0;
  for (int li = 0; li < L; ++li) {
    const double* w = cr.w.data() + (size_t)li * (size_t)p;
    const double* g = cr.g.data() + (size_t)li * (size_t)p;
    double explained = 0.0;
    for (int64_t j = 0; j < p; ++j) explained += w[j] * (cr.c[(size_t)j] - g[j]);
    const double dev = std::max(0.0, yy - (double)n * explained);
    // (a constant response has a null deviance of 0 and nothing to explain: the ratio is 0, not 0 / 0)
    out->dev_ratio[li] = R.null_dev_scaled > 0.0 ? 1.0 - dev / R.null_dev_scaled : 0.0;
    n_sweeps += (double)cr.sweeps[(size_t)li];
    // the intercept at the centres: the response's mean in the preprocessed problem (R.b0); one response (plan_fit: K == 1)
    double b;
    intercepts_at_x_center(X, R, ctl, cr.mean.data(), w, R.b0.data(), &b);
    lambda_done(X, R, path, ctl, li, cr.unconverged[(size_t)li] != 0, w, &b, out);
  }
  out->npasses = n_sweeps;
  pt.mark(wide ? "wcovariance (moments + scale + path)" : "covariance (moments + path)");
  return SGDNET_OK;
}

// ---- several responses (SGDNET_MODE_MCOVARIANCE, covariance.hip) ----
// The features as fit_covariance takes them; the responses as prepare_response left them (standardised only with
// standardize_response) less the null model's intercepts R.b0, subtracted here so that the moments pass multiplies
// deviations.  The intercept of the preprocessed problem stays at R.b0 (less the features' mean shift times w where it
// is fitted), as it does for one response.
// SGDNET_MODE_WMCOVARIANCE is the same stage around wmcovariance_run (S in global memory, any p up to its own limit).
int fit_mcovariance(const Features& X, const Response& R, const Path& path, const FitPlan& plan, const sgdnet_control* ctl,
                    sgdnet_result* out, PhaseTimer& pt) {
  const bool wide = plan.mode == SGDNET_MODE_WMCOVARIANCE;
  const int64_t n = X.n, p = X.p;
  const int L = ctl->n_lambda, K = ctl->n_classes;
  std::vector<double> yd((size_t)n * (size_t)K);
  double yy = 0.0;
  for (int r = 0; r < K; ++r)
    for (int64_t i = 0; i < n; ++i) {
      const double d = R.y[(size_t)(i + (int64_t)r * n)] - R.b0[(size_t)r];
      yd[(size_t)(i + (int64_t)r * n)] = d;
      yy += d * d;
    }
  McovarianceProblem pb;
  fill_problem(pb, X, path, plan, ctl);
  pb.K = K;
  pb.y = yd.data();
  static const int width = exp_env_int("SGDNET_MCOV_WIDTH", 0);     // (64 or 256 lanes: profiles/mcovariance_path.txt)
  McovarianceResult cr;
  const int rc = wide ? wmcovariance_run(pb, &cr, option(kOptWmcovarianceWidth)) : mcovariance_run(pb, &cr, width);
  if (rc) return rc;

  // deviance from the quadratic form, as in fit_covariance: sum_r |y~_r - X~ w_r|^2 = sum_r y~_r'y~_r - n sum_jr w_jr (c~_jr - g_jr)
  const size_t pK = (size_t)p * (size_t)K;
  double n_sweeps = 0.0;
  std::vector<double> b((size_t)K);
  for (int li = 0; li < L; ++li) {
    const double* w = cr.w.data() + (size_t)li * pK;
    const double* g = cr.g.data() + (size_t)li * pK;
    double explained = 0.0;
    for (size_t e = 0; e < pK; ++e) explained += w[e] * (cr.c[e] - g[e]);
    const double dev = std::max(0.0, yy - (double)n * explained);
    out->dev_ratio[li] = R.null_dev_scaled > 0.0 ? 1.0 - dev / R.null_dev_scaled : 0.0;
    n_sweeps += (double)cr.sweeps[(size_t)li];
    intercepts_at_x_center(X, R, ctl, cr.mean.data(), w, R.b0.data(), b.data());
    lambda_done(X, R, path, ctl, li, cr.unconverged[(size_t)li] != 0, w, b.data(), out);
  }
  if (pt.on && wide)
    fprintf(stderr, "[sgdnet]   wmcovariance: moments %.3f ms, scale %.3f ms, path kernel %.3f ms, %.0f sweeps\n", cr.moments_ms, cr.scale_ms,
            cr.path_ms, n_sweeps);
  else if (pt.on)
    fprintf(stderr, "[sgdnet]   mcovariance: moments %.3f ms, path kernel %.3f ms, %.0f sweeps\n", cr.moments_ms, cr.path_ms, n_sweeps);
  out->npasses = n_sweeps;
  pt.mark(wide ? "wmcovariance (moments + scale + path)" : "mcovariance (moments + path)");
  return SGDNET_OK;
}

// ---- Newton mode (SGDNET_MODE_NEWTON, newton.hip) ----
// The same preprocessed problem, for a binomial response: the features centred where fit_covariance centres them, the
// class codes as they came, the intercept an unpenalised coordinate that starts at the null model's value (and stays
// there without an intercept).
// SGDNET_MODE_WNEWTON is the same stage around wnewton_run (H in global memory, any p up to its own limit; sparse x came
// here as its dense copy: fit_sparse_impl).
int fit_newton(const Features& X, const Response& R, const Path& path, const FitPlan& plan, const sgdnet_control* ctl, sgdnet_result* out,
               PhaseTimer& pt) {
  const bool wide = plan.mode == SGDNET_MODE_WNEWTON;
  const int64_t n = X.n, p = X.p;
  const int L = ctl->n_lambda;
  NewtonProblem pb;
  fill_problem(pb, X, path, plan, ctl);
  pb.y = R.y.data();
  pb.fit_intercept = ctl->intercept != 0;
  pb.b0 = R.b0[0];
  NewtonResult nr;
  const int rc = wide ? wnewton_run(pb, pt.on, &nr, option(kOptWnewtonWidth)) : newton_run(pb, pt.on, &nr);
  if (rc) return rc;
  double n_steps = 0.0;
  for (int li = 0; li < L; ++li) {
    const double* u = nr.u.data() + (size_t)li * (size_t)(p + 1);
    // Family::Loss summed over the samples, doubled (families.h; saga_loss_kernel): the state pass left its mean
    out->dev_ratio[li] = 1.0 - 2.0 * (double)n * nr.loss[(size_t)li] / R.null_dev_scaled;
    n_steps += (double)nr.steps[(size_t)li];
    double b;                          // one response (plan_fit: K == 1)
    intercepts_at_x_center(X, R, ctl, nr.mean.data(), u, u + p, &b);
    lambda_done(X, R, path, ctl, li, nr.unconverged[(size_t)li] != 0, u, &b, out);
  }
  if (pt.on && wide)
    fprintf(stderr, "[sgdnet]   wnewton: %.0f outer steps, %.0f state passes (%.0f after a halving), %.0f sweeps; state %.3f ms, moments %.3f ms, "
            "scale %.3f ms, inner solves %.3f ms\n", n_steps, nr.passes, nr.halvings, nr.sweeps, nr.state_ms, nr.moments_ms, nr.scale_ms, nr.cd_ms);
  else if (pt.on)
    fprintf(stderr, "[sgdnet]   newton: %.0f outer steps, %.0f state passes (%.0f after a halving), %.0f sweeps; state %.3f ms, moments %.3f ms, "
            "inner solves %.3f ms\n", n_steps, nr.passes, nr.halvings, nr.sweeps, nr.state_ms, nr.moments_ms, nr.cd_ms);
  out->npasses = nr.passes;
  pt.mark(wide ? "wnewton (state + moments + scale + cd)" : "newton (state + moments + cd)");
  return SGDNET_OK;
}

// ---- multinomial Newton mode (SGDNET_MODE_MNEWTON, mnewton.hip) ----
// The preprocessed problem of fit_newton with K classes: the class codes as they came, per class an unpenalised intercept
// that starts at the null model's value (and stays there without an intercept).  The loss does not see a shift common
// to all intercepts: they are returned with their class mean removed (kkt.py removes the class mean of G0 likewise).
// (sparse x came here as its dense copy: fit_sparse_impl)
// SGDNET_MODE_WMNEWTON is the same stage around wmnewton_run (the joint Hessian in global memory, any p up to its own limit).
int fit_mnewton(const Features& X, const Response& R, const Path& path, const FitPlan& plan, const sgdnet_control* ctl, sgdnet_result* out,
                PhaseTimer& pt) {
  const bool wide = plan.mode == SGDNET_MODE_WMNEWTON;
  const int64_t n = X.n, p = X.p;
  const int L = ctl->n_lambda, K = ctl->n_classes;
  MNewtonProblem pb;
  fill_problem(pb, X, path, plan, ctl);
  pb.K = K;
  pb.y = R.y.data();
  pb.fit_intercept = ctl->intercept != 0;
  pb.b0 = R.b0.data();
  static const int width = exp_env_int("SGDNET_MNEWTON_WIDTH", 0);  // (64 or 256 lanes: profiles/mnewton_path.txt)
  MNewtonResult nr;
  const int rc = wide ? wmnewton_run(pb, pt.on, &nr, option(kOptWmnewtonWidth)) : mnewton_run(pb, pt.on, &nr, width);
  if (rc) return rc;
  const int64_t P = p + 1;
  double n_steps = 0.0;
  std::vector<double> w((size_t)K * (size_t)p), at_centres((size_t)K), b((size_t)K);
  for (int li = 0; li < L; ++li) {
    const double* u = nr.u.data() + (size_t)li * (size_t)(K * P);
    for (int k = 0; k < K; ++k) {
      const double* uk = u + (size_t)k * (size_t)P;
      for (int64_t j = 0; j < p; ++j) w[(size_t)(k + j * K)] = uk[j];
      at_centres[(size_t)k] = uk[p];
    }
    intercepts_at_x_center(X, R, ctl, nr.mean.data(), w.data(), at_centres.data(), b.data());
    double b_mean = 0.0;
    for (int k = 0; k < K; ++k) b_mean += b[(size_t)k];
    b_mean /= (double)K;
    if (ctl->intercept != 0)
      for (int k = 0; k < K; ++k) b[(size_t)k] -= b_mean;
    // Family::Loss summed over the samples, doubled (families.h; saga_loss_kernel): the state pass left its mean
    out->dev_ratio[li] = 1.0 - 2.0 * (double)n * nr.loss[(size_t)li] / R.null_dev_scaled;
    n_steps += (double)nr.steps[(size_t)li];
    lambda_done(X, R, path, ctl, li, nr.unconverged[(size_t)li] != 0, w.data(), b.data(), out);
  }
  if (pt.on && wide)
    fprintf(stderr, "[sgdnet]   wmnewton: %.0f outer steps, %.0f state passes (%.0f after a halving), %.0f sweeps; state %.3f ms, moments %.3f ms, "
            "scale %.3f ms, inner solves %.3f ms\n", n_steps, nr.passes, nr.halvings, nr.sweeps, nr.state_ms, nr.moments_ms, nr.scale_ms, nr.cd_ms);
  else if (pt.on)
    fprintf(stderr, "[sgdnet]   mnewton: %.0f outer steps, %.0f state passes (%.0f after a halving), %.0f sweeps; state %.3f ms, moments %.3f ms, "
            "inner solves %.3f ms\n", n_steps, nr.passes, nr.halvings, nr.sweeps, nr.state_ms, nr.moments_ms, nr.cd_ms);
  out->npasses = nr.passes;
  pt.mark(wide ? "wmnewton (state + moments + scale + cd)" : "mnewton (state + moments + cd)");
  return SGDNET_OK;
}

// ---- what the two cross-validation drivers check alike ----

// count[g] = the rows of group g; every fold[i] is a group id and no group is empty
int count_groups(const int32_t* fold, int64_t n, int n_groups, std::vector<int64_t>& count) {
  count.assign((size_t)n_groups, 0);
  for (int64_t i = 0; i < n; ++i) {
    if (fold[i] < 0 || fold[i] >= n_groups) {
      set_error("fold[%lld] = %d is not a group id in 0..%d", (long long)i, fold[i], n_groups - 1);
      return SGDNET_EINVAL;
    }
    ++count[(size_t)fold[i]];
  }
  for (int g = 0; g < n_groups; ++g)
    if (count[(size_t)g] == 0) {
      set_error("group %d of %d is empty", g, n_groups);
      return SGDNET_EINVAL;
    }
  return SGDNET_OK;
}

// the mixes and their lambdas (n_alpha x L, a row per mix)
int validate_mixes(int n_alpha, const double* alphas, int L, const double* lambdas) {
  for (int a = 0; a < n_alpha; ++a) {
    if (!(alphas[a] >= 0.0 && alphas[a] <= 1.0)) {
      set_error("alphas[%d] = %g is not an elastic-net mix in [0, 1]", a, alphas[a]);
      return SGDNET_EINVAL;
    }
    for (int l = 0; l < L; ++l)
      if (!(lambdas[(size_t)a * L + l] >= 0.0)) {
        set_error("lambdas[%d][%d] = %g is negative", a, l, lambdas[(size_t)a * L + l]);
        return SGDNET_EINVAL;
      }
  }
  return SGDNET_OK;
}

// ---- cross-validation in covariance mode (covariance.hip: covariance_cv_run): the stage behind sgdnet_cv_covariance_* ----
// Every job (mix, training set T) is fit_covariance on x[T], y[T] by definition: the response centred and scaled by its
// moments over T (prepare_response), the features centred (and scaled) by theirs, the penalties of regularization_path
// in the units of that response.  The device assembles all of it from the group moments; what is left for the host is
// the way back to the scale of the data (rescale_values) and the deviance from the quadratic form, per job.
// wide: SGDNET_MODE_WCOVARIANCE, the same stage around wcovariance_cv_run (the stage behind sgdnet_cv_wcovariance_*): its own
// feature limit and byte budget, and no way from one to the other -- each refuses by its own name.
int fit_cv_covariance(CovarianceCvProblem& pb, const sgdnet_control* ctl, const int32_t* fold, int n_groups, int train_on_rest,
                      int n_alpha, const double* alphas, const double* lambdas, sgdnet_cv_cov_result* out, bool wide = false,
                      CovTap* tap = nullptr) {
  const int64_t n = pb.n, p = pb.p;
  const char* entry = wide ? "sgdnet_cv_wcovariance" : "sgdnet_cv_covariance";
  const char* mode = wide ? "wcovariance" : "covariance";
  if (!ctl || !out || !out->a0 || !out->beta || !out->dev_ratio || !out->return_codes || !out->nulldev || !out->npasses || !pb.y ||
      !fold || !alphas || !lambdas) {
    set_error("%s: null pointer", entry);
    return SGDNET_EINVAL;
  }
  if (n <= 0 || p <= 0 || n_groups <= 0 || n_alpha <= 0 || ctl->n_lambda <= 0 || ctl->max_iter == 0 || ctl->tol < 0.0 ||
      (train_on_rest && n_groups < 2)) {
    set_error("%s: invalid size or control field (n, p, n_groups, n_alpha, n_lambda, max_iter, tol; train_on_rest needs two groups)", entry);
    return SGDNET_EINVAL;
  }
  const int L = ctl->n_lambda;
  const int limit = wide ? kWcovMaxFeatures : kCovMaxFeatures;
  const char* what = nullptr;
  if (ctl->family != SGDNET_GAUSSIAN) what = "family = gaussian";
  else if (p > limit) what = wide ? "no more features than sgdnet_wcovariance_max_features()" : "no more features than sgdnet_covariance_max_features()";
  else if (ctl->n_gpus > 1) what = "one GPU (n_gpus <= 1)";
  else if (ctl->debug) what = "debug = 0 (there are no epochs to report losses of)";
  if (what) {
    set_error("mode = %s needs %s: family %d, %lld features (limit %d), n_gpus %d, debug %d", mode, what, ctl->family, (long long)p, limit,
              ctl->n_gpus, ctl->debug);
    return SGDNET_EUNSUPPORTED;
  }
  const size_t moment_bytes = (size_t)n_groups * (size_t)(p + 2) * (size_t)(p + 2) * sizeof(double);
  if (!wide && moment_bytes > kCovGroupMomentBytes) {
    set_error("mode = covariance needs the group moments within %zu bytes: %d groups x (%lld + 2)^2 doubles are %zu bytes",
              kCovGroupMomentBytes, n_groups, (long long)p, moment_bytes);
    return SGDNET_EUNSUPPORTED;
  }
  std::vector<int64_t> count;
  int rc = count_groups(fold, n, n_groups, count);
  if (!rc) rc = validate_mixes(n_alpha, alphas, L, lambdas);
  if (rc) return rc;
  if (wide) {
    // the limits of wcovariance_cv_run that need no device: its grid dimensions and its byte budget
    const bool sparse = pb.x_dense == nullptr;
    const int64_t chunks = sparse ? 0 : group_row_chunks(count.data(), n_groups, cov_rows_per_chunk(n, p + 2, true));
    if (chunks > kCovMaxRowChunks || n_groups > kCovMaxRowChunks) {
      set_error("mode = wcovariance needs at most %d groups and (dense x) row chunks: %d groups, %lld chunks of %lld rows", kCovMaxRowChunks,
                n_groups, (long long)chunks, (long long)n);
      return SGDNET_EUNSUPPORTED;
    }
    const size_t bytes = wcov_cv_bytes(n_groups, p, chunks);
    if (bytes > kWcovCvBytes) {
      set_error("mode = wcovariance needs the moments and the scaled matrices of the groups within %zu bytes: %d groups of %lld features are %zu bytes",
                kWcovCvBytes, n_groups, (long long)p, bytes);
      return SGDNET_EUNSUPPORTED;
    }
  }
  rc = check_device(ctl->device);
  if (rc) return rc;
  PhaseTimer pt;
  const bool intercept = ctl->intercept != 0;
  pb.fold = fold;
  pb.n_groups = n_groups;
  pb.train_on_rest = train_on_rest != 0;
  pb.centre = intercept || ctl->standardize != 0;
  pb.standardize = ctl->standardize != 0;
  pb.device = ctl->device;
  pb.n_mix = n_alpha;
  pb.n_lambda = L;
  pb.mix = alphas;
  pb.lambda = lambdas;
  pb.max_iter = ctl->max_iter;
  pb.tol = ctl->tol;
  CovarianceCvResult cr;
  rc = wide ? wcovariance_cv_run(pb, &cr, option(kOptWcovarianceWidth), tap) : covariance_cv_run(pb, &cr, tap);
  if (rc) return rc;
  if (pt.on)
    fprintf(stderr, "[sgdnet]   cv %s: group moments %.3f ms, assembly %.3f ms, path kernel (%d jobs) %.3f ms\n", mode, cr.moments_ms,
            cr.assemble_ms, n_alpha * n_groups, cr.path_ms);

  // per job, both modes alike: the way back to the scale of the data and the deviance from the quadratic form
  const size_t P = (size_t)p, P1 = P + 1;
  for (int a = 0; a < n_alpha; ++a)
    for (int t = 0; t < n_groups; ++t) {
      const size_t job = (size_t)a * (size_t)n_groups + (size_t)t;
      const double nT = cr.n_train[(size_t)t], ys = cr.y_scale[(size_t)t], yy = cr.yy[(size_t)t];
      const double* mean = cr.mean.data() + (size_t)t * P1;
      const double* scale = cr.scale.data() + (size_t)t * P;
      const double* c = cr.c.data() + job * P;
      double n_sweeps = 0.0;
      for (int li = 0; li < L; ++li) {
        const size_t at = job * (size_t)L + (size_t)li;
        const double* w = cr.w.data() + at * P;
        const double* g = cr.g.data() + at * P;
        double* bo = out->beta + at * P;
        // fit_covariance: the explained part of the deviance is n sum_j w_j (c~_j - g_j); the intercept is the response's
        // mean over T less the features' means times the coefficients, on the scale of the data
        double explained = 0.0, xbb = 0.0;
        for (size_t j = 0; j < P; ++j) {
          explained += w[j] * (c[j] - g[j]);
          bo[j] = w[j] * (ys / scale[j]);
          xbb += mean[j] * bo[j];
        }
        const double dev = std::max(0.0, yy - nT * explained);
        out->dev_ratio[at] = yy > 0.0 ? 1.0 - dev / yy : 0.0;
        out->a0[at] = intercept ? mean[P] - xbb : 0.0;
        out->return_codes[at] = cr.unconverged[at] ? 1.0 : 0.0;
        n_sweeps += (double)cr.sweeps[at];
      }
      out->nulldev[job] = yy * ys * ys;
      out->npasses[job] = n_sweeps;
    }
  pt.mark(wide ? "cv wcovariance (all folds)" : "cv covariance (all folds)");
  return SGDNET_OK;
}

// ---- cross-validation in multi-response covariance mode (covariance.hip: mcovariance_cv_run): the stage behind sgdnet_cv_mcovariance_* ----
// Every job (mix, training set T) is fit_mcovariance on x[T], y[T] by definition: the features centred (and scaled) by their
// moments over T, the responses standardised by theirs only with standardize_response (the fit then stays on that scale:
// mgaussian has y_scale = 1), the null model's intercepts b0_r = mean_T(y~_r) subtracted, the penalties (1 - mix) lambda and
// mix lambda.  The device assembles all of it from the group moments; the host is left with the way back to the scale of
// the features (rescale_values) and the deviance from the quadratic form, per job.
// wide: SGDNET_MODE_WMCOVARIANCE, the same stage around wmcovariance_cv_run (the stage behind sgdnet_cv_wmcovariance_*): its own
// feature limit and byte budget, and no way from one to the other -- each refuses by its own name.
int fit_cv_mcovariance(McovarianceCvProblem& pb, const sgdnet_control* ctl, const int32_t* fold, int n_groups, int train_on_rest,
                       int n_alpha, const double* alphas, const double* lambdas, sgdnet_cv_mcov_result* out, bool wide = false,
                       CovTap* tap = nullptr) {
  const int64_t n = pb.n, p = pb.p;
  const char* entry = wide ? "sgdnet_cv_wmcovariance" : "sgdnet_cv_mcovariance";
  const char* mode = wide ? "wmcovariance" : "mcovariance";
  if (!ctl || !out || !out->a0 || !out->beta || !out->dev_ratio || !out->return_codes || !out->nulldev || !out->npasses || !pb.y ||
      !fold || !alphas || !lambdas) {
    set_error("%s: null pointer", entry);
    return SGDNET_EINVAL;
  }
  if (n <= 0 || p <= 0 || n_groups <= 0 || n_alpha <= 0 || ctl->n_lambda <= 0 || ctl->max_iter == 0 || ctl->tol < 0.0 ||
      (train_on_rest && n_groups < 2)) {
    set_error("%s: invalid size or control field (n, p, n_groups, n_alpha, n_lambda, max_iter, tol; train_on_rest needs two groups)", entry);
    return SGDNET_EINVAL;
  }
  const int L = ctl->n_lambda, K = ctl->n_classes;
  const int limit = wide ? wmcov_max_features(K) : mcov_max_features(K);
  const char* what = nullptr;
  if (ctl->family != SGDNET_MGAUSSIAN) what = "family = mgaussian";
  else if (K < 2) what = "at least two responses (n_classes >= 2)";
  else if (p > limit) what = wide ? "no more features than sgdnet_wmcovariance_max_features(n_classes)" : "no more features than sgdnet_mcovariance_max_features(n_classes)";
  else if (ctl->n_gpus > 1) what = "one GPU (n_gpus <= 1)";
  else if (ctl->debug) what = "debug = 0 (there are no epochs to report losses of)";
  if (what) {
    set_error("mode = %s needs %s: family %d, n_classes %d, %lld features (limit %d), n_gpus %d, debug %d", mode, what, ctl->family, K,
              (long long)p, limit, ctl->n_gpus, ctl->debug);
    return SGDNET_EUNSUPPORTED;
  }
  const size_t moment_bytes = mcov_group_moment_bytes(n_groups, p, K);
  if (!wide && moment_bytes > kCovGroupMomentBytes) {
    set_error("mode = mcovariance needs the group moments within %zu bytes: %d groups x (%lld + %d + 1)^2 doubles are %zu bytes",
              kCovGroupMomentBytes, n_groups, (long long)p, K, moment_bytes);
    return SGDNET_EUNSUPPORTED;
  }
  std::vector<int64_t> count;
  int rc = count_groups(fold, n, n_groups, count);
  if (!rc) rc = validate_mixes(n_alpha, alphas, L, lambdas);
  if (rc) return rc;
  const bool sparse = pb.x_dense == nullptr;
  const int64_t chunks = sparse ? n_groups : group_row_chunks(count.data(), n_groups, cov_rows_per_chunk(n, p + K + 1, wide));
  if (chunks > kCovMaxRowChunks) {
    set_error("mode = %s needs at most %d %s: %d groups of %lld rows are %lld", mode, kCovMaxRowChunks,
              sparse ? "groups of sparse rows" : "row chunks of the groups", n_groups, (long long)n, (long long)chunks);
    return SGDNET_EUNSUPPORTED;
  }
  if (wide) {      // the byte budget of wmcovariance_cv_run (sparse x has no partial tiles)
    const size_t bytes = wmcov_cv_bytes(n_groups, p, K, sparse ? 0 : chunks);
    if (bytes > kWcovCvBytes) {
      set_error("mode = wmcovariance needs the moments and the scaled matrices of the groups within %zu bytes: %d groups of %lld features and %d responses are %zu bytes",
                kWcovCvBytes, n_groups, (long long)p, K, bytes);
      return SGDNET_EUNSUPPORTED;
    }
  }
  rc = check_device(ctl->device);
  if (rc) return rc;
  PhaseTimer pt;
  const bool intercept = ctl->intercept != 0;
  pb.K = K;
  pb.fold = fold;
  pb.n_groups = n_groups;
  pb.train_on_rest = train_on_rest != 0;
  pb.centre = intercept || ctl->standardize != 0;
  pb.standardize = ctl->standardize != 0;
  pb.standardize_response = ctl->standardize_response != 0;
  pb.device = ctl->device;
  pb.n_mix = n_alpha;
  pb.n_lambda = L;
  pb.mix = alphas;
  pb.lambda = lambdas;
  pb.max_iter = ctl->max_iter;
  pb.tol = ctl->tol;
  static const int width = exp_env_int("SGDNET_MCOV_WIDTH", 0);     // (64 or 256 lanes, as fit_mcovariance takes it)
  pb.width = width;
  McovarianceCvResult cr;
  rc = wide ? wmcovariance_cv_run(pb, &cr, option(kOptWmcovarianceWidth), tap) : mcovariance_cv_run(pb, &cr, tap);
  if (rc) return rc;
  if (pt.on)
    fprintf(stderr, "[sgdnet]   cv %s: group moments %.3f ms, assembly %.3f ms, path kernel (%d jobs) %.3f ms\n", mode, cr.moments_ms,
            cr.assemble_ms, n_alpha * n_groups, cr.path_ms);

  // per job, both modes alike: the way back to the scale of the data and the deviance from the quadratic form
  const size_t P = (size_t)p, Ks = (size_t)K, pK = P * Ks;
  std::vector<double> xbb(Ks);
  for (int a = 0; a < n_alpha; ++a)
    for (int t = 0; t < n_groups; ++t) {
      const size_t job = (size_t)a * (size_t)n_groups + (size_t)t;
      const double nT = cr.n_train[(size_t)t], yy = cr.yy[(size_t)t];
      const double* mean = cr.mean.data() + (size_t)t * (P + Ks);
      const double* scale = cr.scale.data() + (size_t)t * P;
      const double* c = cr.c.data() + job * pK;
      double n_sweeps = 0.0;
      for (int li = 0; li < L; ++li) {
        const size_t at = job * (size_t)L + (size_t)li;
        const double* w = cr.w.data() + at * pK;
        const double* g = cr.g.data() + at * pK;
        double* bo = out->beta + at * pK;
        // fit_mcovariance: the explained part of the deviance is n sum_jr w_jr (c~_jr - g_jr); rescale_values with y_scale = 1
        double explained = 0.0;
        std::fill(xbb.begin(), xbb.end(), 0.0);
        for (size_t j = 0; j < P; ++j)
          for (size_t r = 0; r < Ks; ++r) {
            const size_t e = j * Ks + r;
            explained += w[e] * (c[e] - g[e]);
            bo[e] = w[e] * (1.0 / scale[j]);
            xbb[r] += mean[j] * bo[e];
          }
        const double dev = std::max(0.0, yy - nT * explained);
        out->dev_ratio[at] = yy > 0.0 ? 1.0 - dev / yy : 0.0;
        for (size_t r = 0; r < Ks; ++r) out->a0[at * Ks + r] = intercept ? mean[P + r] - xbb[r] : mean[P + r];
        out->return_codes[at] = cr.unconverged[at] ? 1.0 : 0.0;
        n_sweeps += (double)cr.sweeps[at];
      }
      out->nulldev[job] = cr.nulldev[(size_t)t];
      out->npasses[job] = n_sweeps;
    }
  pt.mark(wide ? "cv wmcovariance (all folds)" : "cv mcovariance (all folds)");
  return SGDNET_OK;
}

// ---- what the two Newton cross-validations (fit_cv_newton, fit_cv_mnewton) form alike from a dense x ----

// The rows stably sorted by group: row i goes to position to[i]; start[g] is the first position of group g (G + 1 entries).
void sort_by_group(const int32_t* fold, int64_t n, const std::vector<int64_t>& count, std::vector<int64_t>& start, std::vector<int64_t>& to) {
  const size_t G = count.size();
  start.assign(G + 1, 0);
  for (size_t g = 0; g < G; ++g) start[g + 1] = start[g] + count[g];
  to.resize((size_t)n);
  std::vector<int64_t> fill(start.begin(), start.end() - 1);
  for (int64_t i = 0; i < n; ++i) to[(size_t)i] = fill[(size_t)fold[i]]++;
}

// xs: x (column-major n x p) with its rows sorted; abar: the whole-data column means; s1, s2 (G x p): per group and column
// the sums of d = x - abar and of d^2 (the deviations formed before anything is squared: DESIGN.md 4.6)
void sorted_dense_moments(const double* dense, int64_t n, int64_t p, int G, const std::vector<int64_t>& to, const std::vector<int64_t>& start,
                          std::vector<double>& xs, std::vector<double>& abar, std::vector<double>& s1, std::vector<double>& s2) {
  const size_t P = (size_t)p;
  xs.resize((size_t)n * P);
  parallel_for(p, (double)n * (double)p, [&](int64_t j0, int64_t j1) {
    for (int64_t j = j0; j < j1; ++j) {
      const double* col = dense + j * n;
      double* dst = xs.data() + j * n;
      double sum = 0.0;
      for (int64_t i = 0; i < n; ++i) {
        dst[to[(size_t)i]] = col[i];
        sum += col[i];
      }
      const double a = abar[(size_t)j] = sum / (double)n;
      for (int g = 0; g < G; ++g) {
        double t1 = 0.0, t2 = 0.0;
        for (int64_t i = start[(size_t)g]; i < start[(size_t)g + 1]; ++i) {
          const double d = dst[i] - a;
          t1 += d;
          t2 += d * d;
        }
        s1[(size_t)g * P + (size_t)j] = t1;
        s2[(size_t)g * P + (size_t)j] = t2;
      }
    }
  });
}

// mean, scale (G x p): pooled per training set (the group's own sums, or the total -- added in group order -- less them)
// and moved to the set's own mean: mean_T = a + S1 / n_T, var_T = S2 / n_T - (S1 / n_T)^2
void pooled_centres_and_scales(const std::vector<double>& abar, const std::vector<double>& s1, const std::vector<double>& s2,
                               const std::vector<int64_t>& n_t, bool rest, bool centre, bool standardize, std::vector<double>& mean,
                               std::vector<double>& scale) {
  const size_t P = abar.size();
  const int G = (int)n_t.size();
  mean.assign((size_t)G * P, 0.0);
  scale.assign((size_t)G * P, 1.0);
  for (size_t j = 0; j < P; ++j) {
    const double a = abar[j];
    double t1 = 0.0, t2 = 0.0;
    for (int g = 0; g < G; ++g) {
      t1 += s1[(size_t)g * P + j];
      t2 += s2[(size_t)g * P + j];
    }
    for (int g = 0; g < G; ++g) {
      const double nT = (double)n_t[(size_t)g];
      const double d = (rest ? t1 - s1[(size_t)g * P + j] : s1[(size_t)g * P + j]) / nT;
      const double var = (rest ? t2 - s2[(size_t)g * P + j] : s2[(size_t)g * P + j]) / nT - d * d;
      if (centre) mean[(size_t)g * P + j] = a + d;
      if (standardize) scale[(size_t)g * P + j] = var > 0.0 ? sqrt(var) : 1.0;
    }
  }
}

// ---- cross-validation in Newton mode (newton.hip: newton_cv_run): the stage behind sgdnet_cv_newton_* ----
// Every job (mix, training set T) is fit_newton on x[T], y[T] by definition.  The rows are stably sorted by group here,
// once, so that T is a range of rows or the complement of one; what fit_newton takes from the preprocessing of x[T],
// y[T] -- x_center and x_scale over T, the null model's intercept, the null deviance, regularization_path's penalties
// for the user's lambdas -- is formed here per training set, the features' moments pooled from per-group sums of
// deviations about the whole-data column means (formed before anything is squared: DESIGN.md 4.6).
struct CvNewtonMatrix {
  int64_t n = 0, p = 0;
  const double* dense = nullptr;
  const int32_t* colptr = nullptr;
  const int32_t* rowidx = nullptr;
  const double* values = nullptr;
};

//
// wide (the stage behind sgdnet_cv_wnewton_*, newton.hip: wnewton_cv_run): every job is fit_newton in SGDNET_MODE_WNEWTON on
// x[T], y[T].  The same steps with the wide mode's feature limit and its own workspace bound; sparse x is expanded to the dense
// copy a single wnewton fit makes (driver.cpp: fit_sparse_impl; entries stored twice add up) before anything is computed
// from it and goes the dense way, so a sparse call gives the dense call's bits.  Every refusal is decided before the first
// HIP call; there is no fall-back to the narrow loop or to separate fits.
int fit_cv_newton(const CvNewtonMatrix& X, const double* y, const sgdnet_control* ctl, const int32_t* fold, int n_groups, int train_on_rest,
                  int n_alpha, const double* alphas, const double* lambdas, sgdnet_cv_newton_result* out, bool wide = false) {
  const int64_t n = X.n, p = X.p;
  const char* const who = wide ? "sgdnet_cv_wnewton" : "sgdnet_cv_newton";
  const char* const mode = wide ? "wnewton" : "newton";
  if (!ctl || !out || !out->a0 || !out->beta || !out->dev_ratio || !out->return_codes || !out->nulldev || !out->npasses || !out->steps ||
      !out->halvings || !y || !fold || !alphas || !lambdas) {
    set_error("%s: null pointer", who);
    return SGDNET_EINVAL;
  }
  if (n <= 0 || p <= 0 || n_groups <= 0 || n_alpha <= 0 || ctl->n_lambda <= 0 || ctl->max_iter == 0 || ctl->tol < 0.0 ||
      (train_on_rest && n_groups < 2)) {
    set_error("%s: invalid size or control field (n, p, n_groups, n_alpha, n_lambda, max_iter, tol; train_on_rest needs two groups)", who);
    return SGDNET_EINVAL;
  }
  const int L = ctl->n_lambda, G = n_groups;
  // (wide: x is read dense whichever way it came)
  const bool expand = wide && X.dense == nullptr, sparse = !wide && X.dense == nullptr, rest = train_on_rest != 0;
  const int limit = wide ? kWnewtonMaxFeatures : kNewtonMaxFeatures;
  const char* what = nullptr;
  if (ctl->family != SGDNET_BINOMIAL) what = "family = binomial";
  else if (p > limit) what = wide ? "no more features than sgdnet_wnewton_max_features()" : "no more features than sgdnet_newton_max_features()";
  else if (ctl->n_gpus > 1) what = "one GPU (n_gpus <= 1)";
  else if (ctl->debug) what = "debug = 0 (there are no epochs to report losses of)";
  else if (expand && (double)n * (double)p * 8.0 > (double)kWnewtonDenseCopyBytes)
    what = "the dense copy of a sparse x (n_samples x n_features x 8 bytes) within 1 GiB";
  if (what && wide) {
    set_error("mode = wnewton needs %s: family %d, %lld samples, %lld features (limit %d), n_gpus %d, debug %d", what, ctl->family, (long long)n,
              (long long)p, limit, ctl->n_gpus, ctl->debug);
    return SGDNET_EUNSUPPORTED;
  }
  if (what) {
    set_error("mode = newton needs %s: family %d, %lld features (limit %d), n_gpus %d, debug %d", what, ctl->family, (long long)p,
              kNewtonMaxFeatures, ctl->n_gpus, ctl->debug);
    return SGDNET_EUNSUPPORTED;
  }
  const int width = wide ? option(kOptWnewtonWidth) : 0;
  if (width != 0 && width != kWideNarrow && width != kWideFull) {
    set_error("%s: the option wnewton_width is %d; the inner solve runs on 256 or 1024 lanes (0: the rule)", who, width);
    return SGDNET_EINVAL;
  }
  int rc = validate_response(ctl, y, n);
  if (rc) return rc;
  std::vector<int64_t> count, start, to;
  rc = count_groups(fold, n, G, count);
  if (!rc) rc = validate_mixes(n_alpha, alphas, L, lambdas);
  if (rc) return rc;
  sort_by_group(fold, n, count, start, to);
  std::vector<double> ys((size_t)n);
  for (int64_t i = 0; i < n; ++i) ys[(size_t)to[(size_t)i]] = y[i];
  // the response of every training set: both classes, the null model and its deviance (fit_null_model, null_deviance)
  const bool intercept = ctl->intercept != 0;
  std::vector<int64_t> n_t((size_t)G);
  std::vector<double> b0((size_t)G), nulldev((size_t)G);
  {
    double ones_all = 0.0;
    std::vector<double> ones((size_t)G, 0.0);
    for (int g = 0; g < G; ++g) {
      for (int64_t i = start[(size_t)g]; i < start[(size_t)g + 1]; ++i) ones[(size_t)g] += ys[(size_t)i];
      ones_all += ones[(size_t)g];
    }
    for (int g = 0; g < G; ++g) {
      const int64_t own = start[(size_t)g + 1] - start[(size_t)g];
      n_t[(size_t)g] = rest ? n - own : own;
      const double k = rest ? ones_all - ones[(size_t)g] : ones[(size_t)g];
      if (k <= 0.0 || k >= (double)n_t[(size_t)g]) {
        set_error("the training set of group %d of %d holds one class only (%lld rows, %lld of class 1)", g, G, (long long)n_t[(size_t)g],
                  (long long)k);
        return SGDNET_EINVAL;
      }
      b0[(size_t)g] = intercept ? binomial_link(k / (double)n_t[(size_t)g]) : 0.0;
      // sum over T of log(1 + e^b0) - y b0, its equal terms counted instead of added one by one
      const double lp = b0[(size_t)g];
      nulldev[(size_t)g] = 2.0 * ((double)n_t[(size_t)g] * log(1.0 + exp(lp)) - k * lp);
    }
  }
  if ((int64_t)n_alpha * G > kNewtonCvMaxJobs) {
    set_error("mode = %s needs no more than %lld jobs in one cross-validation call: %d mixes x %d groups", mode, (long long)kNewtonCvMaxJobs,
              n_alpha, G);
    return SGDNET_EUNSUPPORTED;
  }
  const size_t workspace = wide ? wnewton_cv_workspace_bytes(n, p, n_t.data(), G, n_alpha, L)
                                : newton_cv_workspace_bytes(n, p, sparse, n_t.data(), G, n_alpha);
  if (wide && workspace > kWnewtonCvBytes) {
    set_error("mode = wnewton needs the jobs' workspace within %zu bytes: %d mixes x %d groups of %lld rows and %lld features (per job the "
              "moments, the row-chunk partials and H, about 2.5 (features + 2)^2 doubles) are %zu bytes", kWnewtonCvBytes, n_alpha, G,
              (long long)n, (long long)p, workspace);
    return SGDNET_EUNSUPPORTED;
  }
  if (!wide && workspace > kNewtonCvWorkspaceBytes) {
    set_error("mode = newton needs the jobs' workspace within %zu bytes: %d mixes x %d groups of (2 x %lld rows + (%lld + 2)^2 moments%s) "
              "doubles are %zu bytes", kNewtonCvWorkspaceBytes, n_alpha, G, (long long)n, (long long)p, sparse ? "" : " + row-chunk partials",
              workspace);
    return SGDNET_EUNSUPPORTED;
  }
  rc = check_device(ctl->device);
  if (rc) return rc;
  PhaseTimer pt;

  // x with its rows sorted, and per group and column the sums of d = x - a and of d^2 about the whole-data mean a
  const size_t P = (size_t)p;
  std::vector<double> xs, abar(P, 0.0), s1((size_t)G * P, 0.0), s2((size_t)G * P, 0.0);
  std::vector<int32_t> rows, cut;
  if (sparse) {
    const int64_t nnz = X.colptr[p];
    xs.resize((size_t)nnz);
    rows.resize((size_t)nnz);
    cut.resize(P * ((size_t)G + 1));
    std::vector<int64_t> at((size_t)G + 1);
    for (int64_t j = 0; j < p; ++j) {
      const int64_t q0 = X.colptr[j], q1 = X.colptr[j + 1];
      double sum = 0.0;
      for (int64_t q = q0; q < q1; ++q) sum += X.values[q];
      const double a = abar[(size_t)j] = sum / (double)n;
      // a counting pass: the entries of a group keep their order, so the sorted rows ascend within the column
      std::fill(at.begin(), at.end(), 0);
      for (int64_t q = q0; q < q1; ++q) ++at[(size_t)fold[X.rowidx[q]] + 1];
      at[0] = q0;
      for (int g = 0; g < G; ++g) at[(size_t)g + 1] += at[(size_t)g];
      int32_t* c = cut.data() + (size_t)j * ((size_t)G + 1);
      for (int g = 0; g <= G; ++g) c[g] = (int32_t)at[(size_t)g];
      for (int g = 0; g < G; ++g) {     // the rows of the group that store nothing: d = -a
        const double zeros = (double)((start[(size_t)g + 1] - start[(size_t)g]) - (at[(size_t)g + 1] - at[(size_t)g]));
        s1[(size_t)g * P + (size_t)j] = zeros * -a;
        s2[(size_t)g * P + (size_t)j] = zeros * (a * a);
      }
      for (int64_t q = q0; q < q1; ++q) {
        const int32_t r = X.rowidx[q];
        const int g = fold[r];
        const int64_t dst = at[(size_t)g]++;
        rows[(size_t)dst] = (int32_t)to[(size_t)r];
        xs[(size_t)dst] = X.values[q];
        const double d = X.values[q] - a;
        s1[(size_t)g * P + (size_t)j] += d;
        s2[(size_t)g * P + (size_t)j] += d * d;
      }
      // (the pair kernel looks rows up by binary search: a column that came with its rows out of order is put in order)
      bool ascending = true;
      for (int64_t q = q0 + 1; q < q1 && ascending; ++q) ascending = rows[(size_t)q] > rows[(size_t)q - 1];
      if (!ascending) {
        std::vector<std::pair<int32_t, double>> e((size_t)(q1 - q0));
        for (int64_t q = q0; q < q1; ++q) e[(size_t)(q - q0)] = {rows[(size_t)q], xs[(size_t)q]};
        std::stable_sort(e.begin(), e.end(), [](const std::pair<int32_t, double>& l, const std::pair<int32_t, double>& r) { return l.first < r.first; });
        for (int64_t q = q0; q < q1; ++q) {
          rows[(size_t)q] = e[(size_t)(q - q0)].first;
          xs[(size_t)q] = e[(size_t)(q - q0)].second;
        }
      }
    }
  } else if (expand) {
    std::vector<double> expanded((size_t)(n * p), 0.0);
    for (int64_t j = 0; j < p; ++j)
      for (int64_t q = X.colptr[j]; q < X.colptr[j + 1]; ++q) expanded[(size_t)(X.rowidx[q] + j * n)] += X.values[q];
    sorted_dense_moments(expanded.data(), n, p, G, to, start, xs, abar, s1, s2);
  } else {
    sorted_dense_moments(X.dense, n, p, G, to, start, xs, abar, s1, s2);
  }
  const bool centre = intercept || ctl->standardize != 0;
  std::vector<double> mean, scale;
  pooled_centres_and_scales(abar, s1, s2, n_t, rest, centre, ctl->standardize != 0, mean, scale);
  pt.mark(wide ? "cv wnewton: rows sorted, moments" : "cv newton: rows sorted, moments");

  // regularization_path for user lambdas and a binomial response (its y_scale is 1)
  std::vector<double> l2((size_t)n_alpha * (size_t)L), l1(l2.size());
  std::vector<uint8_t> ridge((size_t)n_alpha);
  for (int a = 0; a < n_alpha; ++a) {
    ridge[(size_t)a] = alphas[a] == 0.0;
    for (int l = 0; l < L; ++l) {
      l2[(size_t)a * L + l] = (1.0 - alphas[a]) * lambdas[(size_t)a * L + l] / 1.0;
      l1[(size_t)a * L + l] = alphas[a] * lambdas[(size_t)a * L + l] / 1.0;
    }
  }
  NewtonCvProblem pb;
  pb.n = n;
  pb.p = p;
  if (sparse) {
    pb.colptr = X.colptr;
    pb.rowidx = rows.data();
    pb.values = xs.data();
    pb.cut = cut.data();
  } else {
    pb.x_dense = xs.data();
  }
  pb.y = ys.data();
  pb.n_sets = G;
  pb.start = start.data();
  pb.train_on_rest = rest;
  pb.centre = centre;
  pb.fit_intercept = intercept;
  pb.mean = mean.data();
  pb.scale = scale.data();
  pb.b0 = b0.data();
  pb.device = ctl->device;
  pb.n_mix = n_alpha;
  pb.n_lambda = L;
  pb.l2 = l2.data();
  pb.l1 = l1.data();
  pb.ridge = ridge.data();
  pb.max_iter = ctl->max_iter;
  pb.tol = ctl->tol;
  NewtonCvResult nr;
  rc = wide ? wnewton_cv_run(pb, pt.on, &nr, width) : newton_cv_run(pb, pt.on, &nr);
  if (rc) return rc;

  const size_t P1 = P + 1;
  double most_steps = 0.0, most_halvings = 0.0;
  for (int a = 0; a < n_alpha; ++a)
    for (int t = 0; t < G; ++t) {
      const size_t job = (size_t)a * (size_t)G + (size_t)t;
      const double* m = mean.data() + (size_t)t * P;
      const double* s = scale.data() + (size_t)t * P;
      for (int li = 0; li < L; ++li) {
        const size_t at = job * (size_t)L + (size_t)li;
        const double* u = nr.u.data() + at * P1;
        double* bo = out->beta + at * P;
        // fit_newton and rescale_values: the intercept at the centres less the centres times the coefficients
        double xbb = 0.0;
        for (size_t j = 0; j < P; ++j) {
          bo[j] = u[j] / s[j];
          xbb += m[j] * bo[j];
        }
        out->a0[at] = intercept ? u[P] - xbb : b0[(size_t)t];
        out->dev_ratio[at] = 1.0 - 2.0 * (double)n_t[(size_t)t] * nr.loss[at] / nulldev[(size_t)t];
        out->return_codes[at] = nr.unconverged[at] ? 1.0 : 0.0;
      }
      out->nulldev[job] = nulldev[(size_t)t];
      out->npasses[job] = nr.passes[job];
      out->steps[job] = nr.steps[job];
      out->halvings[job] = nr.halvings[job];
      most_steps = std::max(most_steps, nr.steps[job] + nr.halvings[job]);
      most_halvings = std::max(most_halvings, nr.halvings[job]);
    }
  if (pt.on && wide)
    fprintf(stderr, "[sgdnet]   cv wnewton: %d jobs, %d rounds (the slowest job: %.0f steps + halvings; most halvings %.0f), %.0f sweeps; "
            "moments %.3f ms, scale %.3f ms, inner solves %.3f ms, state %.3f ms\n", n_alpha * G, nr.rounds, most_steps, most_halvings,
            nr.sweeps, nr.moments_ms, nr.scale_ms, nr.cd_ms, nr.state_ms);
  else if (pt.on)
    fprintf(stderr, "[sgdnet]   cv newton: %d jobs, %d rounds (the slowest job: %.0f steps + halvings; most halvings %.0f), %.0f sweeps; "
            "moments %.3f ms, inner solves %.3f ms, state %.3f ms\n", n_alpha * G, nr.rounds, most_steps, most_halvings, nr.sweeps,
            nr.moments_ms, nr.cd_ms, nr.state_ms);
  pt.mark(wide ? "cv wnewton (all folds)" : "cv newton (all folds)");
  return SGDNET_OK;
}

// ---- cross-validation in multinomial Newton mode (mnewton.hip: mnewton_cv_run): the stage behind sgdnet_cv_mnewton_* ----
// Every job (mix, training set T) is fit_mnewton on x[T], y[T] by definition.  Sparse x is expanded to the dense copy a
// single fit makes (driver.cpp: fit_sparse_impl; entries stored twice add up), before anything is computed from it, so a
// sparse call gives the dense call's bits.  Then fit_cv_newton's steps with K classes: the rows sorted, per training set
// x_center and x_scale, the null model's intercepts (the class-centred logs of T's class proportions, or of 1 / K each
// without an intercept) and its deviance, and regularization_path's penalties for the user's lambdas.  A training set
// without a row of some class is refused: its separate fit would silently be a model of fewer classes.
// Every refusal is decided before the first HIP call.
int fit_cv_mnewton(const CvNewtonMatrix& X, const double* y, const sgdnet_control* ctl, const int32_t* fold, int n_groups, int train_on_rest,
                   int n_alpha, const double* alphas, const double* lambdas, sgdnet_cv_mnewton_result* out) {
  const int64_t n = X.n, p = X.p;
  if (!ctl || !out || !out->a0 || !out->beta || !out->dev_ratio || !out->return_codes || !out->nulldev || !out->npasses || !out->steps ||
      !out->halvings || !y || !fold || !alphas || !lambdas) {
    set_error("sgdnet_cv_mnewton: null pointer");
    return SGDNET_EINVAL;
  }
  if (n <= 0 || p <= 0 || n_groups <= 0 || n_alpha <= 0 || ctl->n_lambda <= 0 || ctl->max_iter == 0 || ctl->tol < 0.0 ||
      (train_on_rest && n_groups < 2)) {
    set_error("sgdnet_cv_mnewton: invalid size or control field (n, p, n_groups, n_alpha, n_lambda, max_iter, tol; train_on_rest needs two groups)");
    return SGDNET_EINVAL;
  }
  const int L = ctl->n_lambda, G = n_groups, K = ctl->n_classes;
  const bool sparse = X.dense == nullptr, rest = train_on_rest != 0;
  const int limit = mnewton_max_features(K);
  const char* what = nullptr;
  if (ctl->family != SGDNET_MULTINOMIAL) what = "family = multinomial";
  else if (K < 2 || K >= 100) what = "2 to 99 classes";
  else if (ctl->type_multinomial != 0) what = "the ungrouped penalty (type_multinomial = 0)";
  else if (p > limit) what = "no more features than sgdnet_mnewton_max_features(n_classes)";
  else if (ctl->n_gpus > 1) what = "one GPU (n_gpus <= 1)";
  else if (ctl->debug) what = "debug = 0 (there are no epochs to report losses of)";
  else if (sparse && (double)n * (double)p * 8.0 > (double)kMNewtonDenseCopyBytes)
    what = "the dense copy of a sparse x (n_samples x n_features x 8 bytes) within 1 GiB";
  if (what) {
    set_error("mode = mnewton needs %s: family %d, n_classes %d, %lld samples, %lld features (limit %d), n_gpus %d, debug %d", what, ctl->family,
              K, (long long)n, (long long)p, limit, ctl->n_gpus, ctl->debug);
    return SGDNET_EUNSUPPORTED;
  }
  int rc = validate_response(ctl, y, n);
  if (rc) return rc;
  std::vector<int64_t> count, start, to;
  rc = count_groups(fold, n, G, count);
  if (!rc) rc = validate_mixes(n_alpha, alphas, L, lambdas);
  if (rc) return rc;
  sort_by_group(fold, n, count, start, to);
  std::vector<double> ys((size_t)n);
  for (int64_t i = 0; i < n; ++i) ys[(size_t)to[(size_t)i]] = y[i];
  // the response of every training set: every class, the null model and its deviance (fit_null_model, null_deviance), the
  // equal terms counted instead of added one by one
  const bool intercept = ctl->intercept != 0;
  std::vector<int64_t> n_t((size_t)G);
  std::vector<double> b0((size_t)G * (size_t)K), nulldev((size_t)G);
  {
    std::vector<int64_t> in_group((size_t)G * (size_t)K, 0), in_all((size_t)K, 0);
    for (int g = 0; g < G; ++g)
      for (int64_t i = start[(size_t)g]; i < start[(size_t)g + 1]; ++i) {
        const size_t k = (size_t)(ys[(size_t)i] + 0.5);
        ++in_group[(size_t)g * (size_t)K + k];
        ++in_all[k];
      }
    for (int g = 0; g < G; ++g) {
      const int64_t own = start[(size_t)g + 1] - start[(size_t)g];
      const double nT = (double)(n_t[(size_t)g] = rest ? n - own : own);
      double* b = b0.data() + (size_t)g * (size_t)K;
      double log_sum = 0.0;
      for (int k = 0; k < K; ++k) {
        const int64_t c = rest ? in_all[(size_t)k] - in_group[(size_t)g * (size_t)K + (size_t)k] : in_group[(size_t)g * (size_t)K + (size_t)k];
        if (c <= 0) {
          set_error("the training set of group %d of %d holds no row of class %d (%lld rows)", g, G, k, (long long)n_t[(size_t)g]);
          return SGDNET_EINVAL;
        }
        b[k] = log(intercept ? (double)c / nT : 1.0 / (double)K);
        log_sum += b[k];
      }
      double mx = b[0] - log_sum / (double)K, sum = 0.0, picked = 0.0;
      for (int k = 0; k < K; ++k) {
        b[k] -= log_sum / (double)K;
        mx = std::max(mx, b[k]);
      }
      for (int k = 0; k < K; ++k) {
        const int64_t c = rest ? in_all[(size_t)k] - in_group[(size_t)g * (size_t)K + (size_t)k] : in_group[(size_t)g * (size_t)K + (size_t)k];
        sum += exp(b[k] - mx);
        picked += (double)c * b[k];
      }
      // sum over T of log sum_k e^b_k - b_{y_i}
      nulldev[(size_t)g] = 2.0 * (nT * (log(sum) + mx) - picked);
    }
  }
  const int64_t class_pairs = (int64_t)K * (K + 1) / 2;
  if ((int64_t)n_alpha * G > kNewtonCvMaxJobs || (int64_t)n_alpha * G * class_pairs > kMNewtonCvMaxGridZ) {
    set_error("mode = mnewton needs no more than %lld jobs and %lld jobs x class pairs in one cross-validation call: %d mixes x %d groups "
              "x %lld class pairs", (long long)kNewtonCvMaxJobs, (long long)kMNewtonCvMaxGridZ, n_alpha, G, (long long)class_pairs);
    return SGDNET_EUNSUPPORTED;
  }
  const double workspace = mnewton_cv_workspace_bytes(n, p, K, n_t.data(), G, n_alpha, L);
  if (workspace > (double)kNewtonCvWorkspaceBytes) {
    set_error("mode = mnewton needs the jobs' workspace within %zu bytes: %d mixes x %d groups of (rows x %d classes + %lld class pairs x "
              "((%lld + 2)^2 moments + row-chunk partials) + %d lambdas x %lld coordinates) doubles are %.0f bytes", kNewtonCvWorkspaceBytes,
              n_alpha, G, K, (long long)class_pairs, (long long)p, L, (long long)(K * (p + 1)), workspace);
    return SGDNET_EUNSUPPORTED;
  }
  rc = check_device(ctl->device);
  if (rc) return rc;
  PhaseTimer pt;

  std::vector<double> expanded;
  const double* dense = X.dense;
  if (sparse) {
    expanded.assign((size_t)(n * p), 0.0);
    for (int64_t j = 0; j < p; ++j)
      for (int64_t q = X.colptr[j]; q < X.colptr[j + 1]; ++q) expanded[(size_t)(X.rowidx[q] + j * n)] += X.values[q];
    dense = expanded.data();
  }
  const size_t P = (size_t)p;
  std::vector<double> xs, abar(P, 0.0), s1((size_t)G * P, 0.0), s2((size_t)G * P, 0.0), mean, scale;
  sorted_dense_moments(dense, n, p, G, to, start, xs, abar, s1, s2);
  std::vector<double>().swap(expanded);
  const bool centre = intercept || ctl->standardize != 0;
  pooled_centres_and_scales(abar, s1, s2, n_t, rest, centre, ctl->standardize != 0, mean, scale);
  pt.mark("cv mnewton: rows sorted, moments");

  // regularization_path for user lambdas and a multinomial response (its y_scale is 1)
  std::vector<double> l2((size_t)n_alpha * (size_t)L), l1(l2.size());
  std::vector<uint8_t> ridge((size_t)n_alpha);
  for (int a = 0; a < n_alpha; ++a) {
    ridge[(size_t)a] = alphas[a] == 0.0;
    for (int l = 0; l < L; ++l) {
      l2[(size_t)a * L + l] = (1.0 - alphas[a]) * lambdas[(size_t)a * L + l] / 1.0;
      l1[(size_t)a * L + l] = alphas[a] * lambdas[(size_t)a * L + l] / 1.0;
    }
  }
  MNewtonCvProblem pb;
  pb.n = n;
  pb.p = p;
  pb.K = K;
  pb.x_dense = xs.data();
  pb.y = ys.data();
  pb.n_sets = G;
  pb.start = start.data();
  pb.train_on_rest = rest;
  pb.fit_intercept = intercept;
  pb.mean = mean.data();
  pb.scale = scale.data();
  pb.b0 = b0.data();
  pb.device = ctl->device;
  pb.n_mix = n_alpha;
  pb.n_lambda = L;
  pb.l2 = l2.data();
  pb.l1 = l1.data();
  pb.ridge = ridge.data();
  pb.max_iter = ctl->max_iter;
  pb.tol = ctl->tol;
  MNewtonCvResult nr;
  rc = mnewton_cv_run(pb, pt.on, &nr);
  if (rc) return rc;

  const size_t P1 = P + 1, Q = (size_t)K * P1;
  double most_steps = 0.0, most_halvings = 0.0;
  std::vector<double> b((size_t)K);
  for (int a = 0; a < n_alpha; ++a)
    for (int t = 0; t < G; ++t) {
      const size_t job = (size_t)a * (size_t)G + (size_t)t;
      const double* m = mean.data() + (size_t)t * P;
      const double* s = scale.data() + (size_t)t * P;
      for (int li = 0; li < L; ++li) {
        const size_t at = job * (size_t)L + (size_t)li;
        const double* u = nr.u.data() + at * Q;
        double* bo = out->beta + at * P * (size_t)K;     // entry (k, j) at k + j K
        double* ao = out->a0 + at * (size_t)K;
        // fit_mnewton and rescale_values: per class the intercept at the centres less the centres times the coefficients,
        // then the class mean of the intercepts removed
        double b_mean = 0.0;
        for (int k = 0; k < K; ++k) {
          const double* uk = u + (size_t)k * P1;
          double xbb = 0.0;
          for (size_t j = 0; j < P; ++j) {
            const double v = uk[j] / s[j];
            bo[(size_t)k + j * (size_t)K] = v;
            xbb += m[j] * v;
          }
          b[(size_t)k] = intercept ? uk[P] - xbb : b0[(size_t)t * (size_t)K + (size_t)k];
          b_mean += b[(size_t)k];
        }
        b_mean /= (double)K;
        for (int k = 0; k < K; ++k) ao[k] = intercept ? b[(size_t)k] - b_mean : b[(size_t)k];
        out->dev_ratio[at] = 1.0 - 2.0 * (double)n_t[(size_t)t] * nr.loss[at] / nulldev[(size_t)t];
        out->return_codes[at] = nr.unconverged[at] ? 1.0 : 0.0;
      }
      out->nulldev[job] = nulldev[(size_t)t];
      out->npasses[job] = nr.passes[job];
      out->steps[job] = nr.steps[job];
      out->halvings[job] = nr.halvings[job];
      most_steps = std::max(most_steps, nr.steps[job] + nr.halvings[job]);
      most_halvings = std::max(most_halvings, nr.halvings[job]);
    }
  if (pt.on)
    fprintf(stderr, "[sgdnet]   cv mnewton: %d jobs, %d rounds (the slowest job: %.0f steps + halvings; most halvings %.0f), %.0f sweeps; "
            "moments %.3f ms, inner solves %.3f ms, state %.3f ms\n", n_alpha * G, nr.rounds, most_steps, most_halvings, nr.sweeps,
            nr.moments_ms, nr.cd_ms, nr.state_ms);
  pt.mark("cv mnewton (all folds)");
  return SGDNET_OK;
}

}  // namespace

int sgdnet::fit_direct(const Features& X, const Response& R, const Path& path, const FitPlan& plan, const sgdnet_control* ctl,
                       sgdnet_result* out, PhaseTimer& pt) {
  int rc;
  switch (plan.mode) {
    case SGDNET_MODE_MCOVARIANCE:
    case SGDNET_MODE_WMCOVARIANCE: rc = fit_mcovariance(X, R, path, plan, ctl, out, pt); break;
    case SGDNET_MODE_MNEWTON:
    case SGDNET_MODE_WMNEWTON: rc = fit_mnewton(X, R, path, plan, ctl, out, pt); break;
    case SGDNET_MODE_NEWTON:
    case SGDNET_MODE_WNEWTON: rc = fit_newton(X, R, path, plan, ctl, out, pt); break;
    default: rc = fit_covariance(X, R, path, plan, ctl, out, pt); break;
  }
  if (!rc) out->draws_used = 0;        // no sample is drawn: control.rng_state stays as it came
  return rc;
}

extern "C" {

int sgdnet_cv_covariance_dense(const double* x, int64_t n, int64_t p, const double* y, const int32_t* fold, int n_groups,
                               int train_on_rest, const sgdnet_control* ctl, int n_alpha, const double* alphas, const double* lambdas,
                               sgdnet_cv_cov_result* out) {
  if (!x) {
    set_error("sgdnet_cv_covariance_dense: invalid matrix");
    return SGDNET_EINVAL;
  }
  CovarianceCvProblem pb;
  pb.n = n;
  pb.p = p;
  pb.x_dense = x;
  pb.y = y;
  return fit_cv_covariance(pb, ctl, fold, n_groups, train_on_rest, n_alpha, alphas, lambdas, out);
}

int sgdnet_cv_covariance_sparse(const sgdnet_csc* x, const double* y, const int32_t* fold, int n_groups, int train_on_rest,
                                const sgdnet_control* ctl, int n_alpha, const double* alphas, const double* lambdas,
                                sgdnet_cv_cov_result* out) {
  if (!x || x->n_rows <= 0 || x->n_cols <= 0 || !x->colptr || !x->rowidx || !x->values) {
    set_error("sgdnet_cv_covariance_sparse: invalid matrix");
    return SGDNET_EINVAL;
  }
  int rc;
  if ((rc = validate_colptr(x)) || (rc = validate_rowidx(x))) return rc;
  CovarianceCvProblem pb;
  pb.n = x->n_rows;
  pb.p = x->n_cols;
  pb.colptr = x->colptr;
  pb.rowidx = x->rowidx;
  pb.values = x->values;
  pb.y = y;
  return fit_cv_covariance(pb, ctl, fold, n_groups, train_on_rest, n_alpha, alphas, lambdas, out);
}

int sgdnet_cv_wcovariance_dense(const double* x, int64_t n, int64_t p, const double* y, const int32_t* fold, int n_groups,
                                int train_on_rest, const sgdnet_control* ctl, int n_alpha, const double* alphas, const double* lambdas,
                                sgdnet_cv_cov_result* out) {
  if (!x) {
    set_error("sgdnet_cv_wcovariance_dense: invalid matrix");
    return SGDNET_EINVAL;
  }
  CovarianceCvProblem pb;
  pb.n = n;
  pb.p = p;
  pb.x_dense = x;
  pb.y = y;
  return fit_cv_covariance(pb, ctl, fold, n_groups, train_on_rest, n_alpha, alphas, lambdas, out, true);
}

int sgdnet_cv_wcovariance_sparse(const sgdnet_csc* x, const double* y, const int32_t* fold, int n_groups, int train_on_rest,
                                 const sgdnet_control* ctl, int n_alpha, const double* alphas, const double* lambdas,
                                 sgdnet_cv_cov_result* out) {
  if (!x || x->n_rows <= 0 || x->n_cols <= 0 || !x->colptr || !x->rowidx || !x->values) {
    set_error("sgdnet_cv_wcovariance_sparse: invalid matrix");
    return SGDNET_EINVAL;
  }
  int rc;
  if ((rc = validate_colptr(x)) || (rc = validate_rowidx(x))) return rc;
  CovarianceCvProblem pb;
  pb.n = x->n_rows;
  pb.p = x->n_cols;
  pb.colptr = x->colptr;
  pb.rowidx = x->rowidx;
  pb.values = x->values;
  pb.y = y;
  return fit_cv_covariance(pb, ctl, fold, n_groups, train_on_rest, n_alpha, alphas, lambdas, out, true);
}

int sgdnet_cv_mcovariance_dense(const double* x, int64_t n, int64_t p, const double* y, const int32_t* fold, int n_groups,
                                int train_on_rest, const sgdnet_control* ctl, int n_alpha, const double* alphas, const double* lambdas,
                                sgdnet_cv_mcov_result* out) {
  if (!x) {
    set_error("sgdnet_cv_mcovariance_dense: invalid matrix");
    return SGDNET_EINVAL;
  }
  McovarianceCvProblem pb;
  pb.n = n;
  pb.p = p;
  pb.x_dense = x;
  pb.y = y;
  return fit_cv_mcovariance(pb, ctl, fold, n_groups, train_on_rest, n_alpha, alphas, lambdas, out);
}

int sgdnet_cv_mcovariance_sparse(const sgdnet_csc* x, const double* y, const int32_t* fold, int n_groups, int train_on_rest,
                                 const sgdnet_control* ctl, int n_alpha, const double* alphas, const double* lambdas,
                                 sgdnet_cv_mcov_result* out) {
  if (!x || x->n_rows <= 0 || x->n_cols <= 0 || !x->colptr || !x->rowidx || !x->values) {
    set_error("sgdnet_cv_mcovariance_sparse: invalid matrix");
    return SGDNET_EINVAL;
  }
  int rc;
  if ((rc = validate_colptr(x)) || (rc = validate_rowidx(x))) return rc;
  McovarianceCvProblem pb;
  pb.n = x->n_rows;
  pb.p = x->n_cols;
  pb.colptr = x->colptr;
  pb.rowidx = x->rowidx;
  pb.values = x->values;
  pb.y = y;
  return fit_cv_mcovariance(pb, ctl, fold, n_groups, train_on_rest, n_alpha, alphas, lambdas, out);
}

int sgdnet_cv_wmcovariance_dense(const double* x, int64_t n, int64_t p, const double* y, const int32_t* fold, int n_groups,
                                 int train_on_rest, const sgdnet_control* ctl, int n_alpha, const double* alphas, const double* lambdas,
                                 sgdnet_cv_mcov_result* out) {
  if (!x) {
    set_error("sgdnet_cv_wmcovariance_dense: invalid matrix");
    return SGDNET_EINVAL;
  }
  McovarianceCvProblem pb;
  pb.n = n;
  pb.p = p;
  pb.x_dense = x;
  pb.y = y;
  return fit_cv_mcovariance(pb, ctl, fold, n_groups, train_on_rest, n_alpha, alphas, lambdas, out, true);
}

int sgdnet_cv_wmcovariance_sparse(const sgdnet_csc* x, const double* y, const int32_t* fold, int n_groups, int train_on_rest,
                                  const sgdnet_control* ctl, int n_alpha, const double* alphas, const double* lambdas,
                                  sgdnet_cv_mcov_result* out) {
  if (!x || x->n_rows <= 0 || x->n_cols <= 0 || !x->colptr || !x->rowidx || !x->values) {
    set_error("sgdnet_cv_wmcovariance_sparse: invalid matrix");
    return SGDNET_EINVAL;
  }
  int rc;
  if ((rc = validate_colptr(x)) || (rc = validate_rowidx(x))) return rc;
  McovarianceCvProblem pb;
  pb.n = x->n_rows;
  pb.p = x->n_cols;
  pb.colptr = x->colptr;
  pb.rowidx = x->rowidx;
  pb.values = x->values;
  pb.y = y;
  return fit_cv_mcovariance(pb, ctl, fold, n_groups, train_on_rest, n_alpha, alphas, lambdas, out, true);
}

int sgdnet_cv_newton_dense(const double* x, int64_t n, int64_t p, const double* y, const int32_t* fold, int n_groups, int train_on_rest,
                           const sgdnet_control* ctl, int n_alpha, const double* alphas, const double* lambdas,
                           sgdnet_cv_newton_result* out) {
  if (!x) {
    set_error("sgdnet_cv_newton_dense: invalid matrix");
    return SGDNET_EINVAL;
  }
  CvNewtonMatrix X;
  X.n = n;
  X.p = p;
  X.dense = x;
  return fit_cv_newton(X, y, ctl, fold, n_groups, train_on_rest, n_alpha, alphas, lambdas, out);
}

int sgdnet_cv_newton_sparse(const sgdnet_csc* x, const double* y, const int32_t* fold, int n_groups, int train_on_rest,
                            const sgdnet_control* ctl, int n_alpha, const double* alphas, const double* lambdas,
                            sgdnet_cv_newton_result* out) {
  if (!x || x->n_rows <= 0 || x->n_cols <= 0 || !x->colptr || !x->rowidx || !x->values) {
    set_error("sgdnet_cv_newton_sparse: invalid matrix");
    return SGDNET_EINVAL;
  }
  int rc;
  if ((rc = validate_colptr(x)) || (rc = validate_rowidx(x))) return rc;
  CvNewtonMatrix X;
  X.n = x->n_rows;
  X.p = x->n_cols;
  X.colptr = x->colptr;
  X.rowidx = x->rowidx;
  X.values = x->values;
  return fit_cv_newton(X, y, ctl, fold, n_groups, train_on_rest, n_alpha, alphas, lambdas, out);
}

int sgdnet_cv_wnewton_dense(const double* x, int64_t n, int64_t p, const double* y, const int32_t* fold, int n_groups, int train_on_rest,
                            const sgdnet_control* ctl, int n_alpha, const double* alphas, const double* lambdas,
                            sgdnet_cv_wnewton_result* out) {
  if (!x) {
    set_error("sgdnet_cv_wnewton_dense: invalid matrix");
    return SGDNET_EINVAL;
  }
  CvNewtonMatrix X;
  X.n = n;
  X.p = p;
  X.dense = x;
  return fit_cv_newton(X, y, ctl, fold, n_groups, train_on_rest, n_alpha, alphas, lambdas, out, true);
}

int sgdnet_cv_wnewton_sparse(const sgdnet_csc* x, const double* y, const int32_t* fold, int n_groups, int train_on_rest,
                             const sgdnet_control* ctl, int n_alpha, const double* alphas, const double* lambdas,
                             sgdnet_cv_wnewton_result* out) {
  if (!x || x->n_rows <= 0 || x->n_cols <= 0 || !x->colptr || !x->rowidx || !x->values) {
    set_error("sgdnet_cv_wnewton_sparse: invalid matrix");
    return SGDNET_EINVAL;
  }
  int rc;
  if ((rc = validate_colptr(x)) || (rc = validate_rowidx(x))) return rc;
  CvNewtonMatrix X;
  X.n = x->n_rows;
  X.p = x->n_cols;
  X.colptr = x->colptr;
  X.rowidx = x->rowidx;
  X.values = x->values;
  return fit_cv_newton(X, y, ctl, fold, n_groups, train_on_rest, n_alpha, alphas, lambdas, out, true);
}

int sgdnet_cv_mnewton_dense(const double* x, int64_t n, int64_t p, const double* y, const int32_t* fold, int n_groups, int train_on_rest,
                            const sgdnet_control* ctl, int n_alpha, const double* alphas, const double* lambdas,
                            sgdnet_cv_mnewton_result* out) {
  if (!x) {
    set_error("sgdnet_cv_mnewton_dense: invalid matrix");
    return SGDNET_EINVAL;
  }
  CvNewtonMatrix X;
  X.n = n;
  X.p = p;
  X.dense = x;
  return fit_cv_mnewton(X, y, ctl, fold, n_groups, train_on_rest, n_alpha, alphas, lambdas, out);
}

int sgdnet_cv_mnewton_sparse(const sgdnet_csc* x, const double* y, const int32_t* fold, int n_groups, int train_on_rest,
                             const sgdnet_control* ctl, int n_alpha, const double* alphas, const double* lambdas,
                             sgdnet_cv_mnewton_result* out) {
  if (!x || x->n_rows <= 0 || x->n_cols <= 0 || !x->colptr || !x->rowidx || !x->values) {
    set_error("sgdnet_cv_mnewton_sparse: invalid matrix");
    return SGDNET_EINVAL;
  }
  int rc;
  if ((rc = validate_colptr(x)) || (rc = validate_rowidx(x))) return rc;
  CvNewtonMatrix X;
  X.n = x->n_rows;
  X.p = x->n_cols;
  X.colptr = x->colptr;
  X.rowidx = x->rowidx;
  X.values = x->values;
  return fit_cv_mnewton(X, y, ctl, fold, n_groups, train_on_rest, n_alpha, alphas, lambdas, out);
}

// ---- diagnostics: one outer step of Newton mode (newton.hip: newton_probe) ----

namespace {
// what both probes check after their matrix; the refusals of the plan (fit_plan.hpp) by the same name
int newton_probe_checked(NewtonProblem& pb, int device, sgdnet_newton_probe* io, const char* who) {
  if (!io || !io->y || !io->scale || !io->u_cur || !io->u || io->max_sweeps == 0) {
    set_error("%s: invalid argument", who);
    return SGDNET_EINVAL;
  }
  if (pb.p > kNewtonMaxFeatures) {
    set_error("mode = newton needs no more features than sgdnet_newton_max_features(): %lld features (limit %d)", (long long)pb.p,
              kNewtonMaxFeatures);
    return SGDNET_EUNSUPPORTED;
  }
  const int rc = check_device(device);
  if (rc) return rc;
  pb.y = io->y;
  pb.centre = io->centre != 0;
  pb.scale = io->scale;
  pb.device = device;
  pb.n_lambda = 1;
  return newton_probe(pb, io);
}
}  // namespace

int sgdnet_newton_probe_dense(const double* x, int64_t n, int64_t p, int device, sgdnet_newton_probe* io) {
  if (!x || n <= 0 || p <= 0) {
    set_error("sgdnet_newton_probe_dense: invalid matrix");
    return SGDNET_EINVAL;
  }
  NewtonProblem pb;
  pb.n = n;
  pb.p = p;
  pb.x_dense = x;
  return newton_probe_checked(pb, device, io, "sgdnet_newton_probe_dense");
}

int sgdnet_newton_probe_sparse(const sgdnet_csc* x, int device, sgdnet_newton_probe* io) {
  if (!x || x->n_rows <= 0 || x->n_cols <= 0 || !x->colptr || !x->rowidx || !x->values) {
    set_error("sgdnet_newton_probe_sparse: invalid matrix");
    return SGDNET_EINVAL;
  }
  int rc;
  if ((rc = validate_colptr(x)) || (rc = validate_rowidx(x))) return rc;
  NewtonProblem pb;
  pb.n = x->n_rows;
  pb.p = x->n_cols;
  pb.colptr = x->colptr;
  pb.rowidx = x->rowidx;
  pb.values = x->values;
  return newton_probe_checked(pb, device, io, "sgdnet_newton_probe_sparse");
}

// ---- diagnostics: one outer step of multinomial Newton mode (mnewton.hip: mnewton_probe) ----

namespace {
// the refusals of the plan (fit_plan.hpp) by the same name
int mnewton_probe_checked(MNewtonProblem& pb, int device, sgdnet_mnewton_probe_io* io, const char* who) {
  if (!io || !io->y || !io->scale || !io->u_cur || !io->u || io->K < 2 || io->max_sweeps == 0 ||
      (io->width != 0 && io->width != 64 && io->width != 256)) {
    set_error("%s: invalid argument", who);
    return SGDNET_EINVAL;
  }
  const int limit = mnewton_max_features(io->K);
  if (pb.p > limit) {
    set_error("mode = mnewton needs no more features than sgdnet_mnewton_max_features(n_classes): n_classes %d, %lld features (limit %d)",
              io->K, (long long)pb.p, limit);
    return SGDNET_EUNSUPPORTED;
  }
  const int rc = check_device(device);
  if (rc) return rc;
  pb.K = io->K;
  pb.y = io->y;
  pb.centre = io->centre != 0;
  pb.scale = io->scale;
  pb.fit_intercept = io->fit_intercept != 0;
  pb.device = device;
  pb.n_lambda = 1;
  return mnewton_probe(pb, io);
}
}  // namespace

int sgdnet_mnewton_probe(const double* x, int64_t n, int64_t p, int device, sgdnet_mnewton_probe_io* io) {
  if (!x || n <= 0 || p <= 0) {
    set_error("sgdnet_mnewton_probe: invalid matrix");
    return SGDNET_EINVAL;
  }
  MNewtonProblem pb;
  pb.n = n;
  pb.p = p;
  pb.x_dense = x;
  return mnewton_probe_checked(pb, device, io, "sgdnet_mnewton_probe");
}

// ---- diagnostics: one outer step of the wide Newton modes (newton.hip: wnewton_probe, mnewton.hip: wmnewton_probe) ----
// Every refusal is decided before any HIP call; the limits by the names the plan refuses them by (fit_plan.hpp).

int sgdnet_wnewton_probe(const double* x, int64_t n, int64_t p, int device, sgdnet_wnewton_probe_io* io) {
  if (!x || n <= 0 || p <= 0) {
    set_error("sgdnet_wnewton_probe: invalid matrix");
    return SGDNET_EINVAL;
  }
  if (!io || !io->y || !io->scale || !io->u_cur || !io->u || io->max_sweeps == 0 ||
      (io->width != 0 && io->width != kWideNarrow && io->width != kWideFull)) {
    set_error("sgdnet_wnewton_probe: invalid argument");
    return SGDNET_EINVAL;
  }
  if (p > kWnewtonMaxFeatures) {
    set_error("mode = wnewton needs no more features than sgdnet_wnewton_max_features(): %lld features (limit %d)", (long long)p,
              kWnewtonMaxFeatures);
    return SGDNET_EUNSUPPORTED;
  }
  const int rc = check_device(device);
  if (rc) return rc;
  NewtonProblem pb;
  pb.n = n;
  pb.p = p;
  pb.x_dense = x;
  pb.y = io->y;
  pb.centre = io->centre != 0;
  pb.scale = io->scale;
  pb.device = device;
  pb.n_lambda = 1;
  return wnewton_probe(pb, io);
}

int sgdnet_wmnewton_probe(const double* x, int64_t n, int64_t p, int device, sgdnet_wmnewton_probe_io* io) {
  if (!x || n <= 0 || p <= 0) {
    set_error("sgdnet_wmnewton_probe: invalid matrix");
    return SGDNET_EINVAL;
  }
  if (!io || !io->y || !io->scale || !io->u_cur || !io->u || io->K < 2 || io->max_sweeps == 0 ||
      (io->width != 0 && io->width != kWideNarrow && io->width != kWideFull)) {
    set_error("sgdnet_wmnewton_probe: invalid argument");
    return SGDNET_EINVAL;
  }
  const int limit = wmnewton_max_features(io->K);
  if (p > limit) {
    set_error("mode = wmnewton needs no more features than sgdnet_wmnewton_max_features(n_classes): n_classes %d, %lld features (limit %d)",
              io->K, (long long)p, limit);
    return SGDNET_EUNSUPPORTED;
  }
  const int rc = check_device(device);
  if (rc) return rc;
  MNewtonProblem pb;
  pb.n = n;
  pb.p = p;
  pb.x_dense = x;
  pb.K = io->K;
  pb.y = io->y;
  pb.centre = io->centre != 0;
  pb.scale = io->scale;
  pb.fit_intercept = io->fit_intercept != 0;
  pb.device = device;
  pb.n_lambda = 1;
  return wmnewton_probe(pb, io);
}

}  // extern "C"

// ---- diagnostics: the covariance family stage by stage (covariance.hpp: CovTap) ----
// The handle is the tap itself with its int32 fields converted, so that one getter serves every field.

struct sgdnet_cov_probe {
  CovTap tap;
};

namespace {

// x for a probe: exactly one of the two forms, validated as the fit entry points validate theirs
template <class Problem>
int cov_probe_matrix(Problem& pb, const double* x_dense, const sgdnet_csc* x_sparse, int64_t n, int64_t p, const char* who) {
  if ((x_dense != nullptr) == (x_sparse != nullptr)) {
    set_error("%s: invalid matrix", who);
    return SGDNET_EINVAL;
  }
  if (x_dense) {
    pb.n = n;
    pb.p = p;
    pb.x_dense = x_dense;
    return SGDNET_OK;
  }
  if (x_sparse->n_rows <= 0 || x_sparse->n_cols <= 0 || !x_sparse->colptr || !x_sparse->rowidx || !x_sparse->values) {
    set_error("%s: invalid matrix", who);
    return SGDNET_EINVAL;
  }
  int rc;
  if ((rc = validate_colptr(x_sparse)) || (rc = validate_rowidx(x_sparse))) return rc;
  pb.n = x_sparse->n_rows;
  pb.p = x_sparse->n_cols;
  pb.colptr = x_sparse->colptr;
  pb.rowidx = x_sparse->rowidx;
  pb.values = x_sparse->values;
  return SGDNET_OK;
}

// the feature limit of a mode, refused by the name the plan (fit_plan.hpp) refuses it by
int cov_probe_limit(int64_t p, bool wide, bool multi, int K) {
  const int limit = multi ? (wide ? wmcov_max_features(K) : mcov_max_features(K)) : (wide ? kWcovMaxFeatures : kCovMaxFeatures);
  if (p <= limit) return SGDNET_OK;
  const char* mode = multi ? (wide ? "wmcovariance" : "mcovariance") : (wide ? "wcovariance" : "covariance");
  set_error("mode = %s needs no more features than sgdnet_%s_max_features(%s): %lld features (limit %d)", mode, mode,
            multi ? "n_classes" : "", (long long)p, limit);
  return SGDNET_EUNSUPPORTED;
}

int cov_probe_finish(int rc, sgdnet_cov_probe* h, int ld, sgdnet_cov_probe** out) {
  if (rc) {
    delete h;
    return rc;
  }
  for (const auto& f : h->tap.i32) h->tap.f64[f.first].assign(f.second.begin(), f.second.end());
  if (ld > 0) h->tap.f64["ld"].assign(1, (double)ld);
  *out = h;
  return SGDNET_OK;
}

}  // namespace

extern "C" {

int sgdnet_covariance_path_probe(const double* x_dense, const sgdnet_csc* x_sparse, int64_t n, int64_t p, const double* y, int K,
                                 const double* scale, int centre, int wide, int multi, double mix, int n_lambda, const double* lambda,
                                 int device, double tol, unsigned max_iter, int width, sgdnet_cov_probe** out) {
  if (!out || !y || !scale || !lambda || n_lambda <= 0 || K < 1 || (!multi && K != 1) || !(mix >= 0.0 && mix <= 1.0)) {
    set_error("sgdnet_covariance_probe: invalid argument");
    return SGDNET_EINVAL;
  }
  // the path kernel's workgroup: 0 is the rule a fit follows; the one-response narrow kernel has one width only
  const bool width_ok = width == 0 || (wide ? (width == 256 || width == 1024) : (multi && (width == 64 || width == 256)));
  if (!width_ok || max_iter == 0) {
    set_error("sgdnet_covariance_path_probe: invalid argument");
    return SGDNET_EINVAL;
  }
  std::vector<double> l2((size_t)n_lambda), l1((size_t)n_lambda);
  for (int l = 0; l < n_lambda; ++l) {
    l2[(size_t)l] = (1.0 - mix) * lambda[l];
    l1[(size_t)l] = mix * lambda[l];
  }
  auto fill = [&](DirectProblem& pb) {
    pb.centre = centre != 0;
    pb.scale = scale;
    pb.device = device;
    pb.n_lambda = n_lambda;
    pb.alpha = l2.data();
    pb.beta = l1.data();
    pb.ridge = mix == 0.0;
    pb.max_iter = max_iter;
    pb.tol = tol;
  };
  int rc;
  sgdnet_cov_probe* h = new sgdnet_cov_probe;
  if (multi) {
    McovarianceProblem pb;
    if ((rc = cov_probe_matrix(pb, x_dense, x_sparse, n, p, "sgdnet_covariance_probe")) || (rc = cov_probe_limit(pb.p, wide != 0, true, K)) ||
        (rc = check_device(device)))
      return cov_probe_finish(rc, h, 0, out);
    fill(pb);
    pb.K = K;
    pb.y = y;
    McovarianceResult res;
    rc = wide ? wmcovariance_run(pb, &res, width, &h->tap) : mcovariance_run(pb, &res, width, &h->tap);
    if (!rc && !wide) h->tap.f64["c"] = res.c;
    return cov_probe_finish(rc, h, wide ? (int)wide_leading_dim(pb.p) : 0, out);
  }
  CovarianceProblem pb;
  if ((rc = cov_probe_matrix(pb, x_dense, x_sparse, n, p, "sgdnet_covariance_probe")) || (rc = cov_probe_limit(pb.p, wide != 0, false, 1)) ||
      (rc = check_device(device)))
    return cov_probe_finish(rc, h, 0, out);
  fill(pb);
  pb.y = y;
  CovarianceResult res;
  rc = wide ? wcovariance_run(pb, &res, width, &h->tap) : covariance_run(pb, &res, &h->tap);
  if (!rc && !wide) h->tap.f64["c"] = res.c;
  return cov_probe_finish(rc, h, wide ? (int)wide_leading_dim(pb.p) : 0, out);
}

int sgdnet_covariance_probe(const double* x_dense, const sgdnet_csc* x_sparse, int64_t n, int64_t p, const double* y, int K,
                            const double* scale, int centre, int wide, int multi, double mix, int n_lambda, const double* lambda,
                            int device, sgdnet_cov_probe** out) {
  return sgdnet_covariance_path_probe(x_dense, x_sparse, n, p, y, K, scale, centre, wide, multi, mix, n_lambda, lambda, device, 1e-7, 1000, 0,
                                      out);
}

int sgdnet_cv_covariance_probe(const double* x_dense, const sgdnet_csc* x_sparse, int64_t n, int64_t p, const double* y,
                               const int32_t* fold, int n_groups, int train_on_rest, const sgdnet_control* ctl, int wide, int n_alpha,
                               const double* alphas, const double* lambdas, sgdnet_cov_probe** out) {
  if (!out || !ctl) {
    set_error("sgdnet_cv_covariance_probe: null pointer");
    return SGDNET_EINVAL;
  }
  const bool multi = ctl->family == SGDNET_MGAUSSIAN;
  const char* who = multi ? (wide ? "sgdnet_cv_wmcovariance" : "sgdnet_cv_mcovariance") : (wide ? "sgdnet_cv_wcovariance" : "sgdnet_cv_covariance");
  int rc;
  sgdnet_cov_probe* h = new sgdnet_cov_probe;
  McovarianceCvProblem mpb;
  CovarianceCvProblem cpb;
  if ((rc = multi ? cov_probe_matrix(mpb, x_dense, x_sparse, n, p, who) : cov_probe_matrix(cpb, x_dense, x_sparse, n, p, who)))
    return cov_probe_finish(rc, h, 0, out);
  const int64_t P = multi ? mpb.p : cpb.p;       // (validated: the sparse matrix's own count)
  // the stage's own outputs: sized only where the stage's checks of the sizes and of the feature limit will pass (it refuses
  // the rest before it writes)
  const int K = multi ? ctl->n_classes : 1;
  const int limit = K < 1 ? 0 : multi ? (wide ? wmcov_max_features(K) : mcov_max_features(K)) : (wide ? kWcovMaxFeatures : kCovMaxFeatures);
  const bool sized = n_groups > 0 && n_alpha > 0 && ctl->n_lambda > 0 && P > 0 && P <= limit;
  const size_t jobs = sized ? (size_t)n_alpha * (size_t)n_groups : 1, L = sized ? (size_t)ctl->n_lambda : 1;
  const size_t Ks = sized ? (size_t)K : 1, Ps = sized ? (size_t)P : 1;
  std::vector<double> a0, beta, dev, codes, nulldev, npasses;
  try {
    a0.resize(jobs * L * Ks);
    beta.resize(jobs * L * Ps * Ks);
    dev.resize(jobs * L);
    codes.resize(jobs * L);
    nulldev.resize(jobs);
    npasses.resize(jobs);
  } catch (const std::exception&) {
    set_error("%s: the probe could not allocate its result buffers", who);
    return cov_probe_finish(SGDNET_ENOMEM, h, 0, out);
  }
  if (multi) {
    mpb.y = y;
    sgdnet_cv_mcov_result res{a0.data(), beta.data(), dev.data(), codes.data(), nulldev.data(), npasses.data()};
    rc = fit_cv_mcovariance(mpb, ctl, fold, n_groups, train_on_rest, n_alpha, alphas, lambdas, &res, wide != 0, &h->tap);
    return cov_probe_finish(rc, h, wide ? (int)wide_leading_dim(mpb.p) : 0, out);
  }
  cpb.y = y;
  sgdnet_cv_cov_result res{a0.data(), beta.data(), dev.data(), codes.data(), nulldev.data(), npasses.data()};
  rc = fit_cv_covariance(cpb, ctl, fold, n_groups, train_on_rest, n_alpha, alphas, lambdas, &res, wide != 0, &h->tap);
  return cov_probe_finish(rc, h, wide ? (int)wide_leading_dim(cpb.p) : 0, out);
}

int64_t sgdnet_cov_probe_field(const sgdnet_cov_probe* probe, const char* name, const double** data) {
  if (!probe || !name) return -1;
  const auto it = probe->tap.f64.find(name);
  if (it == probe->tap.f64.end()) return -1;
  if (data) *data = it->second.data();
  return (int64_t)it->second.size();
}

void sgdnet_cov_probe_free(sgdnet_cov_probe* probe) { delete probe; }

}  // extern "C"
