// Lambda-path driver behind sgdnet_fit_sparse / sgdnet_fit_dense.
//
// Mirrors SetupSgdnet (reference src/sgdnet.cpp:119-285): preprocess, lambda
// path, step sizes, then for every lambda {SAGA loop, deviance, rescale} with
// the solver state kept resident in HBM across the path (warm starts,
// src/sgdnet.cpp:187-198).  For sparse x the per-fit O(nnz) setup passes run on
// the device (setup_device.hip; SGDNET_HOST_SETUP=1 keeps the host loops below for
// A/B checks); the SAGA loop and the per-lambda deviance pass run on the GPU and
// there is no CPU fallback.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>

#include "driver_parts.hpp"

using namespace sgdnet;

// ---- what driver_direct.cpp uses too (driver_parts.hpp) ----
namespace sgdnet {

double binomial_link(double ybar) {     // families.h:141-150
  const double pmin = 1e-9, pmax = 1.0 - pmin;
  const double z = ybar > pmax ? pmax : (ybar < pmin ? pmin : ybar);
  return log(z / (1.0 - z));
}

// class codes are used as array indices (FitNullModel, LambdaMax, the gradient kernels)
int validate_response(const sgdnet_control* c, const double* y, int64_t n) {
  if (c->family != SGDNET_BINOMIAL && c->family != SGDNET_MULTINOMIAL) return SGDNET_OK;
  const double top = c->family == SGDNET_BINOMIAL ? 1.0 : (double)(c->n_classes - 1);
  for (int64_t i = 0; i < n; ++i)
    if (!(y[i] >= 0.0 && y[i] <= top && y[i] == floor(y[i]))) {
      set_error("response[%lld] = %g is not a class code in 0..%d", (long long)i, y[i], (int)top);
      return SGDNET_EINVAL;
    }
  return SGDNET_OK;
}

// what the device passes index with: checked before anything is uploaded
int validate_colptr(const sgdnet_csc* x) {
  if (x->colptr[0] != 0) {
    set_error("colptr[0] must be 0");
    return SGDNET_EINVAL;
  }
  for (int64_t j = 0; j < x->n_cols; ++j)
    if (x->colptr[j + 1] < x->colptr[j]) {
      set_error("colptr is not non-decreasing at column %lld", (long long)j);
      return SGDNET_EINVAL;
    }
  return SGDNET_OK;
}

int validate_rowidx(const sgdnet_csc* x) {
  const int64_t nnz = x->colptr[x->n_cols];
  for (int64_t q = 0; q < nnz; ++q) {
    const int32_t r = x->rowidx[q];
    if (r < 0 || r >= x->n_rows) {
      set_error("row index %d out of range at position %lld", r, (long long)q);
      return SGDNET_EINVAL;
    }
  }
  return SGDNET_OK;
}

int check_device(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    set_error("no HIP device available: the SAGA backend has no CPU fallback");
    return SGDNET_ENODEVICE;
  }
  if (device < 0 || device >= ndev) {
    set_error("device %d out of range (%d devices)", device, ndev);
    return SGDNET_EINVAL;
  }
  return SGDNET_OK;
}

void rescale_values(const Features& X, const Response& R, const sgdnet_control* ctl, int li, const double* w, const double* b,
                    sgdnet_result* out) {
  const int K = ctl->n_classes;
  const int64_t p = X.p;
  double* bo = out->beta + (size_t)li * (size_t)(K * p);
  double* ao = out->a0 + (size_t)li * (size_t)K;
  std::vector<double> xbb((size_t)K, 0.0);
  for (int64_t j = 0; j < p; ++j)
    for (int k = 0; k < K; ++k) {
      const double v = w[(size_t)(k + j * K)] * (R.y_scale[(size_t)k] / X.x_scale[(size_t)j]);
      bo[k + j * K] = v;
      xbb[(size_t)k] += X.x_center[(size_t)j] * v;
    }
  for (int k = 0; k < K; ++k)
    ao[k] = ctl->intercept != 0 ? b[(size_t)k] * R.y_scale[(size_t)k] + R.y_center[(size_t)k] - xbb[(size_t)k]
                                : b[(size_t)k];
}

}  // namespace sgdnet

namespace {

// math.h:66-79 Mean / :114-130 StandardDeviation (population sd, 0 -> 1); the columns over a few threads (parallel_for)
void col_mean_sd(const double* x, int64_t n, int64_t m, double* mean, double* sd) {
  parallel_for(m, (double)n * (double)m, [&](int64_t j0, int64_t j1) {
  for (int64_t j = j0; j < j1; ++j) {
    const double* col = x + j * n;
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i) s += col[i];
    mean[j] = s / (double)n;
    double v = 0.0;
    for (int64_t i = 0; i < n; ++i) {
      const double dlt = col[i] - mean[j];
      v += dlt * dlt;
    }
    v /= (double)n;
    sd[j] = (v == 0.0) ? 1.0 : sqrt(v);
  }
  });
}

void standardize_cols(double* x, int64_t n, int64_t m, const double* mean, const double* sd) {
  parallel_for(m, (double)n * (double)m, [&](int64_t j0, int64_t j1) {
    for (int64_t j = j0; j < j1; ++j)
      for (int64_t i = 0; i < n; ++i) x[i + j * n] = (x[i + j * n] - mean[j]) / sd[j];
  });
}

// sample-major copy of a column-major n x p matrix (utils.h:283-288), in cache-sized tiles
void transpose_to_sample_major(const double* xd, int64_t n, int64_t p, double* xt) {
  constexpr int64_t kTile = 64;
  const int64_t row_tiles = (n + kTile - 1) / kTile;
  parallel_for(row_tiles, (double)n * (double)p, [&](int64_t t0, int64_t t1) {
    for (int64_t t = t0; t < t1; ++t) {
      const int64_t i0 = t * kTile, i1 = std::min(n, i0 + kTile);
      for (int64_t j0 = 0; j0 < p; j0 += kTile) {
        const int64_t j1 = std::min(p, j0 + kTile);
        for (int64_t i = i0; i < i1; ++i)
          for (int64_t j = j0; j < j1; ++j) xt[j + i * p] = xd[i + j * n];
      }
    }
  });
}

// x^T v for every feature column; v is n x cols column-major
int xt_times(const Features& X, const double* v, int cols, double* out) {
  if (X.dev) return X.dense_dev ? dense_xt_times(*X.dev, v, cols, out, X.st) : device_xt_times(*X.dev, v, cols, out, X.st);
  for (int c = 0; c < cols; ++c) {
    const double* vc = v + (int64_t)c * X.n;
    parallel_for(X.p, X.sparse ? 0.0 : (double)X.n * (double)X.p, [&](int64_t j0, int64_t j1) {
      for (int64_t j = j0; j < j1; ++j) {
        double s = 0.0;
        if (X.sparse) {
          for (int64_t q = X.colptr[j]; q < X.colptr[j + 1]; ++q) s += X.val[(size_t)q] * vc[X.rowidx[q]];
        } else {
          const double* col = X.xd.data() + j * X.n;
          for (int64_t i = 0; i < X.n; ++i) s += col[i] * vc[i];
        }
        out[j + (int64_t)c * X.p] = s;
      }
    });
  }
  return SGDNET_OK;
}

double log_sum_exp_host(const double* x, int K) {
  double mx = x[0];
  for (int k = 1; k < K; ++k) mx = std::max(mx, x[k]);
  double s = 0.0;
  for (int k = 0; k < K; ++k) s += exp(x[k] - mx);
  return log(s) + mx;
}

// Family::FitNullModel (families.h:112-117,190-201,287-298,380-385); yt is Ky x n
void fit_null_model(int family, int K, const double* yt, int Ky, int64_t n, bool fit_intercept,
                    double* b0) {
  if (family == SGDNET_GAUSSIAN || family == SGDNET_MGAUSSIAN) {
    for (int k = 0; k < Ky; ++k) {
      double s = 0.0;
      for (int64_t i = 0; i < n; ++i) s += yt[k + i * Ky];
      b0[k] = s / (double)n;
    }
  } else if (family == SGDNET_BINOMIAL) {
    if (fit_intercept) {
      double s = 0.0;
      for (int64_t i = 0; i < n; ++i) s += yt[i];
      b0[0] = binomial_link(s / (double)n);
    } else {
      b0[0] = 0.0;
    }
  } else {
    if (fit_intercept) {
      for (int k = 0; k < K; ++k) b0[k] = 0.0;
      for (int64_t i = 0; i < n; ++i) b0[(int64_t)(yt[i] + 0.5)] += 1.0 / (double)n;
    } else {
      for (int k = 0; k < K; ++k) b0[k] = 1.0 / (double)K;
    }
    double ls = 0.0;
    for (int k = 0; k < K; ++k) ls += log(b0[k]);
    for (int k = 0; k < K; ++k) b0[k] = log(b0[k]) - ls / (double)K;
  }
}

// Family::NullDeviance (families.h:98-110,170-188,262-285,367-378); yt is Ky x n
double null_deviance(int family, int K, const double* yt, int Ky, int64_t n, bool fit_intercept) {
  std::vector<double> lp((size_t)std::max(K, Ky));
  double loss = 0.0;
  if (family == SGDNET_GAUSSIAN || family == SGDNET_MGAUSSIAN) {
    fit_null_model(family, K, yt, Ky, n, true, lp.data());
    for (int64_t i = 0; i < n; ++i) {
      double s = 0.0;
      for (int k = 0; k < Ky; ++k) {
        const double dlt = lp[(size_t)k] - yt[k + i * Ky];
        s += dlt * dlt;
      }
      loss += 0.5 * s;
    }
  } else if (family == SGDNET_BINOMIAL) {
    fit_null_model(family, K, yt, Ky, n, fit_intercept, lp.data());
    for (int64_t i = 0; i < n; ++i) loss += log(1.0 + exp(lp[0])) - yt[i] * lp[0];
  } else {
    fit_null_model(family, K, yt, Ky, n, fit_intercept, lp.data());
    const double lse = log_sum_exp_host(lp.data(), K);
    for (int64_t i = 0; i < n; ++i) loss += lse - lp[(size_t)(unsigned)(yt[i] + 0.5)];
  }
  return 2.0 * loss;
}

// Family::LambdaMax (families.h:119-126,203-220,300-325,387-406); y is n x Ky, preprocessed
double lambda_max(int family, int K, const Features& X, const double* y, int Ky, const double* y_scale) {
  const int64_t n = X.n, p = X.p;
  double best = 0.0;
  if (family == SGDNET_GAUSSIAN) {
    std::vector<double> xty((size_t)p);
    if (xt_times(X, y, 1, xty.data())) return NAN;
    for (int64_t j = 0; j < p; ++j) best = std::max(best, fabs(xty[(size_t)j]));
    return y_scale[0] * best / (double)n;
  }
  if (family == SGDNET_BINOMIAL) {
    double ybar, ystd;
    col_mean_sd(y, n, 1, &ybar, &ystd);
    std::vector<double> ymap((size_t)n), xty((size_t)p);
    for (int64_t i = 0; i < n; ++i) ymap[(size_t)i] = (y[i] - ybar) / ystd;
    if (xt_times(X, ymap.data(), 1, xty.data())) return NAN;
    for (int64_t j = 0; j < p; ++j) best = std::max(best, fabs(xty[(size_t)j]));
    return ystd * best / (double)n;
  }
  if (family == SGDNET_MULTINOMIAL) {
    std::vector<double> ymap((size_t)(n * K), 0.0), xty((size_t)(p * K)), ybar((size_t)K), ystd((size_t)K);
    for (int64_t i = 0; i < n; ++i) ymap[(size_t)(i + (int64_t)(unsigned)(y[i] + 0.5) * n)] = 1.0;
    col_mean_sd(ymap.data(), n, K, ybar.data(), ystd.data());
    standardize_cols(ymap.data(), n, K, ybar.data(), ystd.data());
    if (xt_times(X, ymap.data(), K, xty.data())) return NAN;
    for (int k = 0; k < K; ++k)
      for (int64_t j = 0; j < p; ++j)
        best = std::max(best, fabs(xty[(size_t)(j + (int64_t)k * p)] * ystd[(size_t)k]));
    return best / (double)n;
  }
  std::vector<double> ymap(y, y + n * Ky), xty((size_t)(p * Ky)), ybar((size_t)Ky), ystd((size_t)Ky);
  col_mean_sd(y, n, Ky, ybar.data(), ystd.data());
  standardize_cols(ymap.data(), n, Ky, ybar.data(), ystd.data());
  if (xt_times(X, ymap.data(), Ky, xty.data())) return NAN;
  for (int64_t j = 0; j < p; ++j) {
    double s = 0.0;
    for (int k = 0; k < Ky; ++k) {
      const double v = xty[(size_t)(j + (int64_t)k * p)] * (y_scale[k] * ystd[(size_t)k]);
      s += v * v;
    }
    best = std::max(best, sqrt(s));
  }
  return best / (double)n;
}

// Where the sample order comes from (include/sgdnet_hip.h "sample order").
struct DrawSource {
  const sgdnet_control* ctl;
  sgdnet_rng rng;
  int64_t pos = 0;
  explicit DrawSource(const sgdnet_control* c) : ctl(c) {
    if (c->rng_state) rng = *c->rng_state;
    else sgdnet_rng_seed(&rng, c->seed);
  }
  void finish() const {
    if (internal() && ctl->rng_state) *ctl->rng_state = rng;
  }
  bool internal() const { return !ctl->sample_stream && !ctl->unif; }
  double next_unif() {
    if (!ctl->unif) return sgdnet_rng_unif(&rng);
    double u;
    do {
      u = ctl->unif(ctl->unif_ctx);
    } while (u <= 0.0 || u >= 1.0);
    return u;
  }
  // One epoch of `count` draws over n samples.  shards > 1: the layout the virtual-shard kernels
  // read (include/sgdnet_hip.h: sgdnet_solver_set_virtual_shards) -- count / shards entries per
  // shard, shard after shard, entry t of shard v drawn uniformly from shard v's sample range; the
  // generator is still advanced by exactly `count` uniforms, like the reference's epoch.
  int fill(uint32_t n, uint32_t* out, int64_t count, int shards = 1) {
    if (ctl->sample_stream) {
      if (pos + count > ctl->sample_stream_len) {
        set_error("explicit sample stream exhausted: %lld draws requested, %lld supplied",
                  (long long)(pos + count), (long long)ctl->sample_stream_len);
        return SGDNET_ESTREAM;
      }
      for (int64_t i = 0; i < count; ++i) {
        const uint32_t v = ctl->sample_stream[pos + i];
        if (v >= n) {
          set_error("sample_stream[%lld] = %u is not a sample index (n_samples = %u)", (long long)(pos + i), v, n);
          return SGDNET_EINVAL;
        }
        out[i] = v;
      }
    } else if (shards > 1) {
      const int64_t dps = count / shards, base = (int64_t)n / shards, rem = (int64_t)n % shards;
      int64_t i = 0;
      for (int v = 0; v < shards; ++v) {
        const int64_t lo = (int64_t)v * base + std::min<int64_t>(v, rem);
        const double size = (double)(base + (v < rem ? 1 : 0));
        for (int64_t t = 0; t < dps; ++t) out[i++] = (uint32_t)(lo + (int64_t)floor(size * next_unif()));
      }
      for (; i < count; ++i) {       // positions no shard consumes
        (void)next_unif();
        out[i] = 0;
      }
    } else if (ctl->unif) {
      const double nd = (double)n;
      for (int64_t i = 0; i < count; ++i) out[i] = (uint32_t)floor(nd * next_unif());
    } else {
      sgdnet_rng_fill(&rng, n, out, count);
    }
    pos += count;
    return SGDNET_OK;
  }
};


// The strided sample of the rows L_F is estimated from: 2e6 elements per step, at least 1000 rows -- but never more
// than 16M elements (1000 rows of 10^6 features would be 8 GB)
struct RowSample {
  int64_t stride, m;
};
RowSample gram_row_sample(int64_t n, int64_t p) {
  const int64_t m_max = std::max<int64_t>(8, std::max<int64_t>(std::min<int64_t>(1000, 16000000 / p), 2000000 / p));
  const int64_t stride = (n + m_max - 1) / m_max;
  return {stride, (n + stride - 1) / stride};
}

// largest eigenvalue of Xs'Xs / m (power iteration) for the m x p sample Xs(r, j) = x[j * ld + r * stride]:
// a column-major sample of its own (ld = m, stride = 1), or every stride-th row of a column-major n x p matrix (ld = n)
double sample_gram_lmax(const double* x, size_t ld, size_t stride, size_t m, size_t p) {
  std::vector<double> v(p, 1.0 / std::sqrt((double)p)), w(p), u(m);
  double lmax = 0.0;
  for (int it = 0; it < 30; ++it) {
    std::fill(u.begin(), u.end(), 0.0);
    for (size_t j = 0; j < p; ++j) {
      const double* col = x + j * ld;
      const double vj = v[j];
      for (size_t r = 0; r < m; ++r) u[r] += col[r * stride] * vj;
    }
    double nrm = 0.0;
    for (size_t j = 0; j < p; ++j) {
      const double* col = x + j * ld;
      double sacc = 0.0;
      for (size_t r = 0; r < m; ++r) sacc += col[r * stride] * u[r];
      w[j] = sacc / (double)m;
      nrm += w[j] * w[j];
    }
    nrm = std::sqrt(nrm);
    if (!(nrm > 0.0)) break;
    const double prev = lmax;
    lmax = nrm;
    for (size_t j = 0; j < p; ++j) v[j] = w[j] / nrm;
    if (it >= 3 && std::fabs(lmax - prev) <= 2e-3 * lmax) break;
  }
  return lmax;
}

// L_F of x held on the host: the largest eigenvalue of X'X/n, or a lower bound of it
double host_l_f(const Features& X) {
  // largest mean squared feature value = largest diagonal entry of X'X/n
  double diag = 0.0;
  for (int64_t j = 0; j < X.p; ++j) {
    double s = 0.0;
    if (X.sparse) {
      for (int64_t q = X.colptr[j]; q < X.colptr[j + 1]; ++q) s += X.val[(size_t)q] * X.val[(size_t)q];
    } else {
      const double* col = X.xd.data() + (size_t)j * (size_t)X.n;
      for (int64_t i = 0; i < X.n; ++i) s += col[i] * col[i];
    }
    diag = std::max(diag, s / (double)X.n);
  }
  // The diagonal only bounds the largest eigenvalue of X'X/n from below; strongly collinear
  // columns (abalone: 8 size measurements of one animal) have an L_F several times their
  // diagonal and the window comes out that many times too long.  For small dense x the Gram
  // matrix is cheap: power iteration gives the eigenvalue itself.
  if (!X.sparse && (double)X.n * (double)X.p * (double)X.p <= 2e8 && X.p > 1) {
    const size_t p = (size_t)X.p, n = (size_t)X.n;
    std::vector<double> G(p * p, 0.0), v(p, 1.0), u(p);
    for (size_t j = 0; j < p; ++j)
      for (size_t k = 0; k <= j; ++k) {
        const double *a = X.xd.data() + j * n, *b = X.xd.data() + k * n;
        double s = 0.0;
        for (size_t i = 0; i < n; ++i) s += a[i] * b[i];
        G[j * p + k] = G[k * p + j] = s / (double)n;
      }
    double lmax = 0.0;
    for (int it = 0; it < 200; ++it) {
      double nu = 0.0;
      for (size_t j = 0; j < p; ++j) {
        double s = 0.0;
        for (size_t k = 0; k < p; ++k) s += G[j * p + k] * v[k];
        u[j] = s;
        nu += s * s;
      }
      nu = std::sqrt(nu);
      if (!(nu > 0.0)) break;
      const double prev = lmax;
      lmax = nu;                                   // |G v| with |v| = 1
      for (size_t j = 0; j < p; ++j) v[j] = u[j] / nu;
      if (it > 5 && std::fabs(lmax - prev) <= 1e-6 * lmax) break;
      if (it == 0) lmax = 0.0;                     // v was not normalised yet
    }
    diag = std::max(diag, lmax);
  } else if (!X.sparse && X.p > 1) {
    // larger dense x: the same power iteration through X itself, over evenly spaced rows
    const RowSample rows = gram_row_sample(X.n, X.p);
    diag = std::max(diag, sample_gram_lmax(X.xd.data(), (size_t)X.n, (size_t)rows.stride, (size_t)rows.m, (size_t)X.p));
  }
  return diag;
}

int validate(const sgdnet_control* c, const sgdnet_result* out, int y_cols) {
  if (!c || !out || !out->a0 || !out->beta || !out->lambda || !out->dev_ratio || !out->return_codes) {
    set_error("null control/result pointer");
    return SGDNET_EINVAL;
  }
  if (c->family < SGDNET_GAUSSIAN || c->family > SGDNET_MGAUSSIAN) {
    set_error("unknown family %d", c->family);
    return SGDNET_EINVAL;
  }
  if (c->n_lambda <= 0 || c->n_classes <= 0 || c->max_iter == 0 || c->tol < 0.0 ||
      c->elasticnet_mix < 0.0 || c->elasticnet_mix > 1.0) {
    set_error("invalid control field (n_lambda, n_classes, max_iter, tol or elasticnet_mix)");
    return SGDNET_EINVAL;
  }
  if (c->n_lambda_user > 0 && (c->n_lambda_user != c->n_lambda || !c->lambda)) {
    set_error("control.lambda must hold n_lambda values");
    return SGDNET_EINVAL;
  }
  if (c->family == SGDNET_MGAUSSIAN ? (y_cols != c->n_classes) : (y_cols != 1)) {
    set_error("response has %d columns, family expects %d", y_cols,
              c->family == SGDNET_MGAUSSIAN ? c->n_classes : 1);
    return SGDNET_EINVAL;
  }
  if (c->debug && !c->losses_sink && (!out->losses || !out->losses_len)) {
    set_error("control.debug needs control.losses_sink, or result.losses and result.losses_len");
    return SGDNET_EINVAL;
  }
  return SGDNET_OK;
}

// ---- the stages of a fit (fit_common below is their list) ----

using Clock = std::chrono::steady_clock;
double since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }
struct PathTimes {   // SGDNET_TRACE: where the path's time goes
  double rng = 0.0, run = 0.0, chk = 0.0, dev = 0.0;
};

// the response as the solvers see it; *nulldev = the null deviance of the response as it came
Response prepare_response(const double* y_in, int64_t n, int Ky, const sgdnet_control* ctl, double* nulldev) {
  const int family = ctl->family, K = ctl->n_classes;
  const bool fit_intercept = ctl->intercept != 0;
  Response R;
  R.y.assign(y_in, y_in + n * Ky);
  R.yt.resize((size_t)(n * Ky));
  R.y_center.assign((size_t)K, 0.0);
  R.y_scale.assign((size_t)K, 1.0);
  auto transpose_y = [&]() {
    for (int64_t i = 0; i < n; ++i)
      for (int k = 0; k < Ky; ++k) R.yt[(size_t)(k + i * Ky)] = R.y[(size_t)(i + (int64_t)k * n)];
  };

  transpose_y();
  *nulldev = null_deviance(family, K, R.yt.data(), Ky, n, fit_intercept);        // sgdnet.cpp:154

  if (family == SGDNET_GAUSSIAN) {                                               // families.h:68-79
    col_mean_sd(R.y.data(), n, 1, R.y_center.data(), R.y_scale.data());
    for (int64_t i = 0; i < n; ++i) R.y[(size_t)i] = (R.y[(size_t)i] - R.y_center[0]) / R.y_scale[0];
  } else if (family == SGDNET_MGAUSSIAN && ctl->standardize_response) {          // families.h:337-348
    std::vector<double> m((size_t)Ky), s((size_t)Ky);
    col_mean_sd(R.y.data(), n, Ky, m.data(), s.data());
    standardize_cols(R.y.data(), n, Ky, m.data(), s.data());
  }
  transpose_y();                                                                 // sgdnet.cpp:178

  R.b0.assign((size_t)K, 0.0);
  fit_null_model(family, K, R.yt.data(), Ky, n, fit_intercept, R.b0.data());     // sgdnet.cpp:210
  R.null_dev_scaled = null_deviance(family, K, R.yt.data(), Ky, n, fit_intercept);   // :211
  return R;
}

// RegularizationPath: utils.h:142-181
int regularization_path(const sgdnet_control* ctl, const Features& X, const Response& R, int Ky, Path& path) {
  const int n_lambda = ctl->n_lambda;
  const double mix = ctl->elasticnet_mix;
  path.lambda.resize((size_t)n_lambda);
  path.alpha.resize((size_t)n_lambda);
  path.beta.resize((size_t)n_lambda);
  if (ctl->n_lambda_user == 0) {
    const double lmax = lambda_max(ctl->family, ctl->n_classes, X, R.y.data(), Ky, R.y_scale.data()) / std::max(mix, 0.001);
    if (std::isnan(lmax)) return SGDNET_EHIP;   // device pass failed (sgdnet_last_error says why)
    if (lmax != 0.0) {
      const double log_from = log(lmax);
      const double step = (log(lmax * ctl->lambda_min_ratio) - log_from) / (double)(n_lambda - 1);
      for (int i = 0; i < n_lambda; ++i) path.lambda[(size_t)i] = exp(log_from + i * step);
    } else {
      std::fill(path.lambda.begin(), path.lambda.end(), 0.0);
    }
  } else {
    std::copy(ctl->lambda, ctl->lambda + n_lambda, path.lambda.begin());
  }
  const double max_scale = *std::max_element(R.y_scale.begin(), R.y_scale.end());
  for (int i = 0; i < n_lambda; ++i) {
    path.alpha[(size_t)i] = (1.0 - mix) * path.lambda[(size_t)i] / max_scale;
    path.beta[(size_t)i] = mix * path.lambda[(size_t)i] / max_scale;
  }
  return SGDNET_OK;
}

// ColNormsMax (utils.h:60-85) for the four layouts of x.  The device layouts finish their setup here, and where
// the automatic window will need L_F they sample it on the way (into X.dev_max_mean_sq).
int row_norm_max(Features& X, const sgdnet_control* ctl, const Response& R, int Ky, bool trace, double* norm_max) {
  const int64_t n = X.n, p = X.p;
  *norm_max = 0.0;
  if (X.dev && X.dense_dev) {
    // L_F for the automatic window from a strided sample of the standardised rows (<= 2e6 elements), while
    // the column-major copy is still there; then transpose + row norms on the device
    if (device_setup_wants_l_f(*ctl) && p > 1) {
      const RowSample rows = gram_row_sample(n, p);
      std::vector<double> xs((size_t)(rows.m * p));
      int rcd = dense_sample_rows(*X.dev, rows.stride, rows.m, xs.data(), X.st);
      if (rcd) return rcd;
      X.dev_max_mean_sq = std::max(X.dev_max_mean_sq, sample_gram_lmax(xs.data(), (size_t)rows.m, 1, (size_t)rows.m, (size_t)p));
    }
    return dense_setup_finish(*X.dev, X.st, norm_max);
  }
  if (X.dev) {
    // transpose, row norms and record packing on the device; y rides inside the records
    static const int align = exp_env_int("SGDNET_REC_ALIGN", 128);
    int rcd = device_setup_finish(*X.dev, R.yt.data(), Ky, ctl->standardize ? 1 : 0, align, X.st, norm_max);
    if (rcd) return rcd;
    if (device_setup_wants_l_f(*ctl) && option(kOptWindowEigenvalue)) {   // the automatic window needs L_F itself
      double lmax = 0.0;
      rcd = device_gram_lmax(*X.dev, ctl->standardize ? 1 : 0, X.st, &lmax);
      if (rcd) return rcd;
      if (trace)
        fprintf(stderr, "[sgdnet]   L_F: largest eigenvalue of X'X/n %.4g, its diagonal bound %.4g\n", lmax,
                X.dev_max_mean_sq);
      X.dev_max_mean_sq = std::max(X.dev_max_mean_sq, lmax);
    }
    return SGDNET_OK;
  }
  if (X.sparse) {
    double csq = 0.0;
    if (ctl->standardize)
      for (int64_t j = 0; j < p; ++j) csq += X.x_center_scaled[(size_t)j] * X.x_center_scaled[(size_t)j];
    for (int64_t i = 0; i < n; ++i) {
      double nrm = 0.0, cnz = 0.0;
      for (int64_t q = X.sptr[(size_t)i]; q < X.sptr[(size_t)i + 1]; ++q) {
        if (ctl->standardize) {
          const double cj = X.x_center_scaled[(size_t)X.sidx[(size_t)q]];
          const double dlt = X.sval[(size_t)q] - cj;
          nrm += dlt * dlt;
          cnz += cj * cj;
        } else {
          nrm += X.sval[(size_t)q] * X.sval[(size_t)q];
        }
      }
      if (ctl->standardize) nrm += csq - cnz;
      *norm_max = std::max(*norm_max, nrm);
    }
    return SGDNET_OK;
  }
  for (int64_t i = 0; i < n; ++i) {
    double nrm = 0.0;
    for (int64_t j = 0; j < p; ++j) nrm += X.xt[(size_t)(j + i * p)] * X.xt[(size_t)(j + i * p)];
    *norm_max = std::max(*norm_max, nrm);
  }
  return SGDNET_OK;
}

// The ranks of a fit: one solver per GPU the fit is sharded over (one, unless control.n_gpus > 1).  ss[0] leads.
// Owns the solvers and, while it is open, their sample-order pipeline.
struct Ranks {
  std::vector<sgdnet_solver*> ss;
  bool pipe_open = false;
  Ranks() = default;
  Ranks(const Ranks&) = delete;
  Ranks& operator=(const Ranks&) = delete;
  ~Ranks() {
    sgdnet_rng scratch;
    if (pipe_open)
      for (sgdnet_solver* s : ss) (void)solver_rng_close(s, &scratch);
    for (sgdnet_solver* s : ss) sgdnet_solver_destroy(s);
  }
  sgdnet_solver* lead() const { return ss[0]; }
  int count() const { return (int)ss.size(); }
  // f(solver, rank) on every rank, until one fails
  template <class F>
  int each(F f) {
    for (size_t q = 0; q < ss.size(); ++q) {
      const int r = f(ss[q], (int)q);
      if (r) return r;
    }
    return SGDNET_OK;
  }
};

// One solver adopting the device setup, or one per rank over its slice of the host copy
int create_ranks(const Features& X, const sgdnet_control* ctl, const Response& R, int Ky, const FitPlan& plan, Ranks& ranks) {
  const int64_t n = X.n;
  sgdnet_problem pb{};
  pb.family = ctl->family;
  pb.n_classes = ctl->n_classes;
  pb.n_samples = n;
  pb.n_total = n;
  pb.n_features = X.p;
  pb.fit_intercept = ctl->intercept != 0 ? 1 : 0;
  pb.standardize = (X.sparse && ctl->standardize) ? 1 : 0;
  if (X.dev) {
    // matrix (and for sparse x the centring vector and records) are adopted from the device setup
  } else if (X.sparse) {
    pb.rowptr = X.sptr.data();
    pb.colidx = X.sidx.data();
    pb.values = X.sval.data();
    pb.x_center_scaled = pb.standardize ? X.x_center_scaled.data() : nullptr;
  } else {
    pb.x_dense = X.xt.data();
  }
  pb.y = R.yt.data();
  pb.y_rows = Ky;
  pb.device = ctl->device;

  if (plan.n_ranks == 1) {
    sgdnet_solver* s = nullptr;
    const int rc = X.dev ? solver_create_adopting(&pb, *X.dev, &s) : sgdnet_solver_create(&pb, &s);
    if (rc) return rc;
    ranks.ss.push_back(s);
    return SGDNET_OK;
  }
  std::vector<int64_t> ptr_q;
  for (int q = 0; q < plan.n_ranks; ++q) {
    const int64_t lo = plan.rank_lo[(size_t)q], hi = plan.rank_lo[(size_t)q + 1];
    sgdnet_problem pq = pb;
    pq.n_samples = hi - lo;
    pq.n_total = hi - lo;                       // local normalisation: a rank's shards average their own samples
    ptr_q.assign(X.sptr.begin() + lo, X.sptr.begin() + hi + 1);
    const int64_t off = ptr_q[0];
    for (int64_t& v : ptr_q) v -= off;
    pq.rowptr = ptr_q.data();
    pq.colidx = X.sidx.data() + off;
    pq.values = X.sval.data() + off;
    pq.y = R.yt.data() + lo * Ky;
    pq.device = plan.rank_dev[(size_t)q];
    sgdnet_solver* sq = nullptr;
    const int rc = sgdnet_solver_create(&pq, &sq);
    if (rc) return rc;
    ranks.ss.push_back(sq);
  }
  return SGDNET_OK;
}

// Asks the solvers for the shards of the plan and links the ranks; *applied = the shards the fit runs with
int apply_shards(Ranks& ranks, const FitPlan& plan, const ShardPlan& sp, int* applied) {
  *applied = 0;
  if (sp.shards > 0 && plan.n_ranks > 1) {
    int rc = ranks.each([&](sgdnet_solver* s, int q) {
      int r = sp.cu_budget[(size_t)q] ? sgdnet_solver_set_cu_budget(s, sp.cu_budget[(size_t)q]) : SGDNET_OK;
      if (!r) r = sgdnet_solver_set_virtual_shards(s, sp.shards);
      if (!r) r = sgdnet_solver_set_merge_period(s, sp.merge_period);
      return r;
    });
    if (!rc) rc = sgdnet_solver_link_peers(ranks.ss.data(), plan.n_ranks);
    if (rc) return rc;
    *applied = sp.shards;
  } else if (sp.shards > 0) {
    const int rc = sgdnet_solver_set_virtual_shards(ranks.lead(), sp.shards);
    if (rc && rc != SGDNET_EUNSUPPORTED) return rc;   // SGDNET_EUNSUPPORTED: no sharded form for this problem, the fit goes on without
    if (!rc) *applied = sp.shards;
  }
  if (plan.n_ranks > 1 && *applied < 2) {
    set_error("control.n_gpus = %d: the sample order cannot be laid out per shard (explicit sample_stream?)", plan.n_ranks);
    return SGDNET_EUNSUPPORTED;
  }
  return SGDNET_OK;
}

// The sample order of a fit: where the draws come from and how many of them were consumed
struct SampleOrder {
  DrawSource draws;
  DrawKind kind;
  // DrawKind::kEpochBlocks -- Exact mode with the built-in generator: the draws come in BLOCKS of several epochs
  // (generated on the device, ~1M draws at a time) and one launch runs as many epochs as the block still holds,
  // with the convergence test in the kernel -- a small problem (iris: 150 draws per epoch) is then no
  // longer one launch + one host round trip per epoch.  The stream is consumed contiguously across
  // epochs and lambdas, so the generator ends exactly where the reference's would: the final state is
  // the block's start state stepped by the draws that were used.
  struct {
    sgdnet_rng start;
    int64_t cap = 0, used = 0;
    bool have = false;
  } blk;
  int64_t blk_epochs;
  std::vector<uint32_t> chunk;   // DrawKind::kHost: one epoch of draws
  SampleOrder(const sgdnet_control* ctl, DrawKind k, int64_t n)
      : draws(ctl), kind(k), blk_epochs(block_epochs(n)), chunk(k == DrawKind::kHost ? (size_t)n : 0) {}
};

// DrawKind::kPipeline -- built-in generator: the draws are produced in HBM (r_rng_device.hip), one epoch ahead of
// the epoch that consumes them, on a side stream (solver.cpp: solver_rng_*)
int open_pipeline(Ranks& ranks, const FitPlan& plan, int64_t n, int gens, SampleOrder& so) {
  if (plan.n_ranks == 1) {
    int rc = solver_rng_open(ranks.lead(), &so.draws.rng, n, gens);
    if (rc) return rc;
    ranks.pipe_open = true;
    return solver_rng_prefetch(ranks.lead());
  }
  // ONE R stream over all ranks: an epoch is n consecutive draws of set.seed()'s generator, rank q takes the
  // n_q of them that start lo_q draws in -- its generators start there (the caller's state jumped lo_q draws,
  // mt_jump.cpp) and move n draws per epoch like everybody's.  Rank 0's state after the fit is R's after
  // epochs * n draws: what one GPU returns.
  ranks.pipe_open = true;
  return ranks.each([&](sgdnet_solver* s, int q) {
    sgdnet_rng start = so.draws.rng;
    if (plan.rank_lo[(size_t)q] > 0) {
      std::vector<uint32_t> poly(624);
      if (!mt_jump_poly((uint64_t)plan.rank_lo[(size_t)q], poly.data())) {
        set_error("control.n_gpus: the jump polynomial of the generator could not be formed");
        return (int)SGDNET_EHIP;
      }
      mt_jump_host(&so.draws.rng, poly.data(), &start);
    }
    const int64_t nq = plan.rank_lo[(size_t)q + 1] - plan.rank_lo[(size_t)q];
    int rc = solver_rng_open(s, &start, nq, gens, n);
    if (!rc) rc = solver_rng_prefetch(s);
    return rc;
  });
}

// the end of the sample order: the generator state after exactly the draws that were used goes back to the caller
int close_sample_order(Ranks& ranks, SampleOrder& so, int64_t n) {
  if (so.kind == DrawKind::kPipeline) {
    ranks.pipe_open = false;
    int rc = ranks.each([&](sgdnet_solver* s, int q) {
      sgdnet_rng other;
      return solver_rng_close(s, q == 0 ? &so.draws.rng : &other);   // (rank 0:) state after exactly the epochs that ran
    });
    if (rc) return rc;
  }
  if (so.kind == DrawKind::kEpochBlocks && so.blk.have) {                    // state after exactly the draws that were used
    so.draws.rng = so.blk.start;
    std::vector<uint32_t> scratch((size_t)std::max<int64_t>(1, so.blk.used));
    if (so.blk.used > 0) sgdnet_rng_fill(&so.draws.rng, (uint32_t)n, scratch.data(), so.blk.used);
  }
  so.draws.finish();
  return SGDNET_OK;
}

// One epoch on several ranks: every rank's epoch is enqueued before any of them is waited for (the ranks' kernels
// wait for each other), then ConvergenceCheck on every rank; *converged is the leading rank's
int epoch_all_ranks(Ranks& ranks, const FitPlan& plan, const sgdnet_control* ctl, int64_t n, int64_t batch, SampleOrder& so,
                    PathTimes& t, int* converged) {
  auto t0 = Clock::now();
  int64_t offs[8] = {0};
  int rc = ranks.each([&](sgdnet_solver* s, int q) {
    const int r = solver_rng_prefetch(s);
    return r ? r : solver_rng_acquire(s, &offs[q]);
  });
  if (rc) return rc;
  so.draws.pos += n;
  t.rng += since(t0);
  t0 = Clock::now();
  rc = ranks.each([&](sgdnet_solver* s, int q) {
    return sgdnet_solver_enqueue_epochs(s, batch, offs[q], plan.rank_lo[(size_t)q + 1] - plan.rank_lo[(size_t)q], 1);
  });
  if (!rc) rc = ranks.each([&](sgdnet_solver* s, int) { return solver_rng_release(s); });
  // ConvergenceCheck on every rank: the same coefficients everywhere, each rank keeps its own w_prev
  if (!rc) rc = ranks.each([&](sgdnet_solver* s, int q) {
    int cq = 0;
    const int r = sgdnet_solver_convergence(s, ctl->tol, &cq);
    if (q == 0) *converged = cq;
    if (!r && solver_fused_aborted(s)) {
      set_error("control.n_gpus = %d: rank %d's epoch kernel could not run (its GPU is shared with other work, or "
                "the ranks' kernels did not get to run side by side)", plan.n_ranks, q);
      return (int)SGDNET_EHIP;
    }
    return r;
  });
  if (rc) return rc;
  t.run += since(t0);
  return SGDNET_OK;
}

struct EpochRun {
  unsigned ran = 0;            // epochs that ran (several where the draws come in blocks)
  int converged = 0;
  bool bin_overflow = false;   // the epoch is void: a bin of the binned form overflowed
};

// Epochs of the single solver: exactly the draws the reference would consume are taken from the source (R's RNG
// state after the call matches, SURVEY.md 8b "RNG").  `epochs` of this lambda have run; losses: control.debug
int epoch_one_solver(sgdnet_solver* S, const FitPlan& plan, const sgdnet_control* ctl, int64_t n, int64_t batch, int shards,
                     unsigned epochs, SampleOrder& so, std::vector<double>& losses, PathTimes& t, EpochRun* run) {
  const bool pipe = so.kind == DrawKind::kPipeline, blocks = so.kind == DrawKind::kEpochBlocks;
  int64_t stream_off = 0;
  unsigned want_epochs = 1;
  auto t0 = Clock::now();
  int rc = SGDNET_OK;
  if (blocks) {
    auto& blk = so.blk;
    if (!blk.have || blk.cap - blk.used < n) {
      blk.start = so.draws.rng;
      blk.cap = so.blk_epochs * n;
      blk.used = 0;
      blk.have = true;
      rc = sgdnet_solver_generate_stream(S, &so.draws.rng, blk.cap);   // draws.rng <- state after the block
      if (rc) return rc;
    }
    stream_off = blk.used;
    want_epochs = (unsigned)std::min<int64_t>((blk.cap - blk.used) / n, (int64_t)(ctl->max_iter - epochs));
  } else if (pipe) {
    rc = solver_rng_prefetch(S);               // next epoch's draws, concurrently
    if (rc) return rc;
    rc = solver_rng_acquire(S, &stream_off);   // this epoch's
    so.draws.pos += n;
  } else {
    rc = so.draws.fill((uint32_t)n, so.chunk.data(), n, shards > 1 ? shards : 1);
    if (rc) return rc;
    rc = sgdnet_solver_upload_stream(S, so.chunk.data(), n);
  }
  if (rc) return rc;
  t.rng += since(t0);
  t0 = Clock::now();
  if (ctl->debug && losses.size() < (size_t)epochs + 1) losses.resize(std::max<size_t>(64, 2 * losses.size()));
  rc = sgdnet_solver_run(S, plan.mode, batch, stream_off, n, want_epochs, ctl->tol, &run->ran, &run->converged,
                         ctl->debug ? losses.data() + epochs : nullptr);
  if (rc == SGDNET_EUNSUPPORTED && solver_bin_overflowed(S)) {
    run->bin_overflow = true;
    return pipe ? solver_rng_release(S) : SGDNET_OK;
  }
  if (rc) return rc;
  if (blocks) {
    so.blk.used += (int64_t)run->ran * n;
    so.draws.pos += (int64_t)run->ran * n;
  }
  if (pipe) {
    rc = solver_rng_release(S);
    if (rc) return rc;
  }
  t.run += since(t0);
  return SGDNET_OK;
}

// (batched mode) what the leading rank's last epoch did to the coefficients, handed to the guard
int check_epoch(sgdnet_solver* S, const sgdnet_control* ctl, WindowGuard& guard, int li, unsigned epochs, std::vector<double>& b,
                GuardAction* act) {
  double ch = 0.0, sz = 0.0;
  sgdnet_solver_last_change(S, &ch, &sz);
  // the soft threshold maps a NaN coefficient to 0, so a blown-up run can look converged
  // (max|w| = 0): the intercept keeps the evidence
  bool finite = std::isfinite(WindowGuard::change_ratio(ch, sz)) && std::isfinite(sz);
  if (finite && ctl->intercept != 0) {
    const int rc = sgdnet_solver_get_state(S, 1, b.data());
    if (rc) return rc;
    for (int k = 0; k < ctl->n_classes; ++k) finite = finite && std::isfinite(b[(size_t)k]);
  }
  *act = guard.epoch_ended(li, epochs, ch, sz, finite);
  return SGDNET_OK;
}

// Performs what the guard returned.  kAgain: the shards go where it says so (one GPU only), and every rank starts
// from the null model again; *again tells the caller.  kFail: the error is set and its code returned.
int obey(const GuardAction& act, Ranks& ranks, const double* b0, bool trace, bool* batched_gave_up, bool* again) {
  *again = false;
  if (trace && !act.note.empty()) fprintf(stderr, "[sgdnet]   %s\n", act.note.c_str());
  if (act.what == GuardAction::kFail) {
    if (!act.message.empty()) set_error("%s", act.message.c_str());
    *batched_gave_up = act.gave_up;
    return act.code;
  }
  if (act.what == GuardAction::kGoOn) return SGDNET_OK;
  if (act.drop_shards) {
    const int rc = sgdnet_solver_set_virtual_shards(ranks.lead(), 0);
    if (rc) return rc;
  }
  *again = true;
  return ranks.each([&](sgdnet_solver* s, int) { return solver_reset_state(s, b0); });
}

// the deviance of the training data: every rank adds that of its samples (sgdnet.cpp:246-256)
int deviance_all_ranks(Ranks& ranks, double* dev) {
  *dev = 0.0;
  return ranks.each([&](sgdnet_solver* s, int) {
    double dq = 0.0;
    const int r = sgdnet_solver_deviance(s, &dq);
    *dev += dq;
    return r;
  });
}

int rescale_into(sgdnet_solver* S, const Features& X, const Response& R, const sgdnet_control* ctl, int li, std::vector<double>& w,
                 std::vector<double>& b, sgdnet_result* out) {
  int rc = sgdnet_solver_get_state(S, 0, w.data());
  if (rc) return rc;
  rc = sgdnet_solver_get_state(S, 1, b.data());
  if (rc) return rc;
  rescale_values(X, R, ctl, li, w.data(), b.data(), out);
  return SGDNET_OK;
}

// *batched_gave_up: the batched iteration gave up on this fit (mode = auto then runs it again in exact mode)
int fit_common(Features& X, const double* y_in, int Ky, const sgdnet_control* ctl, sgdnet_result* out, bool* batched_gave_up) {
  const int K = ctl->n_classes;
  const int64_t n = X.n, p = X.p;
  const bool fit_intercept = ctl->intercept != 0;
  *batched_gave_up = false;

  FitFacts facts;
  if (hipGetDeviceCount(&facts.n_devices) != hipSuccess || facts.n_devices <= 0) {
    set_error("no HIP device available: the SAGA backend has no CPU fallback");
    return SGDNET_ENODEVICE;
  }
  PhaseTimer pt;
  const bool trace = pt.on;

  // ---- prepare: response, lambda path, row norms (SetupSgdnet's preprocessing) ----
  Response R = prepare_response(y_in, n, Ky, ctl, &out->nulldev);
  Path path;
  int rc = regularization_path(ctl, X, R, Ky, path);
  if (rc) return rc;
  if (plans_direct(ctl->mode)) {      // plan_fit says whether it may run; it needs none of the SAGA setup below
    facts.ctl = ctl;
    facts.sparse = X.sparse;
    facts.on_device = X.dev != nullptr;
    facts.n = n;
    facts.p = p;
    const FitPlan plan = plan_fit(facts);
    if (plan.rc) {
      set_error("%s", plan.error.c_str());
      return plan.rc;
    }
    return fit_direct(X, R, path, plan, ctl, out, pt);       // driver_direct.cpp
  }
  double norm_max = 0.0;
  rc = row_norm_max(X, ctl, R, Ky, trace, &norm_max);
  if (rc) return rc;
  const double L_scaling = (ctl->family == SGDNET_GAUSSIAN || ctl->family == SGDNET_MGAUSSIAN) ? 1.0 : 0.25;

  // ---- plan (fit_plan.hpp) ----
  facts.ctl = ctl;
  facts.sparse = X.sparse;
  facts.on_device = X.dev != nullptr;
  facts.n = n;
  facts.p = p;
  facts.norm_max = norm_max;
  facts.opt.virtual_shards = option(kOptVirtualShards);
  facts.opt.rng_generators = option(kOptRngGenerators);
  facts.opt.exact_epoch_blocks = option(kOptExactEpochBlocks);
  if (X.dev) facts.l_f = X.dev_max_mean_sq;
  else if (wants_l_f(*ctl)) facts.l_f = host_l_f(X);   // (a pass over x, or its Gram matrix: only for the fits that need it)
  FitPlan plan = plan_fit(facts);
  if (plan.window_refused && trace)
    fprintf(stderr, "[sgdnet]   mode = auto: window rule gives %.1f draws (%lld batches per epoch): exact iteration\n",
            plan.raw_window, (long long)plan.batches_per_epoch);
  if (plan.rc) {
    set_error("%s", plan.error.c_str());
    return plan.rc;
  }
  pt.mark("response, path, step sizes");

  // ---- create the ranks; what only the solvers know goes back into the plan ----
  Ranks ranks;
  rc = create_ranks(X, ctl, R, Ky, plan, ranks);
  if (rc) return rc;
  sgdnet_solver* S = ranks.lead();     // every rank holds the same coefficients after an epoch: the path's decisions are taken from S
  pt.mark("solver create (pack + H2D)");
  rc = ranks.each([&](sgdnet_solver* s, int) { return sgdnet_solver_set_state(s, 1, R.b0.data()); });
  if (rc) return rc;
  if (plan.mode == SGDNET_MODE_BATCHED && K > 16 && !solver_batched_available(S, plan.window)) {
    if (ctl->mode == SGDNET_MODE_BATCHED && trace)
      fprintf(stderr, "[sgdnet]   %d classes on %lld features: no batched form, exact iteration\n", K, (long long)p);
    take_exact_iteration(plan, facts);
  }
  int shards = 0;
  rc = apply_shards(ranks, plan, plan_shards(plan, facts), &shards);
  if (rc) return rc;
  WindowGuard guard(*ctl, plan, shard_window(plan, facts, shards), shards, R.null_dev_scaled);

  // ---- open the draws ----
  SampleOrder so(ctl, plan.draws, n);
  if (so.kind == DrawKind::kPipeline) {
    rc = open_pipeline(ranks, plan, n, generators_per_rank(plan, facts), so);
    if (rc) return rc;
  }

  std::vector<double> w((size_t)(K * p)), b((size_t)K);
  std::vector<double> losses;        // debug: grows with the epochs run, like the reference's vector (saga-sparse.h:364)
  double n_iter = 0.0;
  PathTimes t;
  for (int li = 0; li < ctl->n_lambda; ++li) {                                   // sgdnet.cpp:217-273
    // StepSize: utils.h:31-51
    const double alpha = path.alpha[(size_t)li];
    const double L = (norm_max + (fit_intercept ? 1.0 : 0.0)) * L_scaling + alpha;
    const double mu_n = 2.0 * (double)n * alpha;
    const double gamma = 1.0 / (2.0 * L + std::min(L, mu_n));
    rc = ranks.each([&](sgdnet_solver* s, int) { return sgdnet_solver_set_penalty(s, plan.penalty, gamma, alpha, path.beta[(size_t)li]); });
    if (rc) return rc;

    unsigned epochs = 0;
    int converged = 0;
    bool again = false;
    guard.lambda_starts();
    if (li == 0 && trace) fprintf(stderr, "[sgdnet]   window %lld draws\n", (long long)guard.window());
    while (epochs < ctl->max_iter && !converged) {
      EpochRun run;
      if (plan.n_ranks > 1) {
        run.ran = 1;
        rc = epoch_all_ranks(ranks, plan, ctl, n, guard.window(), so, t, &run.converged);
      } else {
        rc = epoch_one_solver(S, plan, ctl, n, guard.window(), guard.shards(), epochs, so, losses, t, &run);
      }
      if (rc) return rc;
      const auto t0 = Clock::now();
      GuardAction act;
      if (run.bin_overflow) {
        act = guard.bin_overflowed(li, solver_grow_bins(S));
      } else {
        epochs += run.ran;
        converged = run.converged;
        if (plan.mode == SGDNET_MODE_BATCHED) rc = check_epoch(S, ctl, guard, li, epochs, b, &act);
        if (rc) return rc;
      }
      rc = obey(act, ranks, R.b0.data(), trace, batched_gave_up, &again);
      if (rc) return rc;
      if (again) {
        if (act.new_budget) epochs = 0;
        converged = 0;
      }
      t.chk += since(t0);
    }
    const auto t1 = Clock::now();
    out->return_codes[li] = (epochs == ctl->max_iter) ? 1.0 : 0.0;               // saga-sparse.h:376-382

    double dev = 0.0;
    rc = deviance_all_ranks(ranks, &dev);
    if (rc) return rc;
    const bool decreasing = li > 0 && path.lambda[(size_t)li] < path.lambda[(size_t)li - 1];
    rc = obey(guard.lambda_ended(li, dev, decreasing), ranks, R.b0.data(), trace, batched_gave_up, &again);
    if (rc) return rc;
    if (again) {
      --li;
      continue;
    }
    n_iter += (double)epochs;          // epochs of the accepted run of this lambda only
    if (ctl->debug) {
      if (ctl->losses_sink) ctl->losses_sink(ctl->losses_ctx, li, losses.data(), (int)epochs);
      if (out->losses && out->losses_len) {
        memcpy(out->losses + (size_t)li * ctl->max_iter, losses.data(), sizeof(double) * epochs);
        out->losses_len[li] = (int32_t)epochs;
      }
    }
    out->dev_ratio[li] = 1.0 - dev / R.null_dev_scaled;                          // :258
    out->lambda[li] = path.lambda[(size_t)li];
    rc = rescale_into(S, X, R, ctl, li, w, b, out);
    if (rc) return rc;
    t.dev += since(t1);
  }
  if (trace)
    fprintf(stderr, "[sgdnet]   of which: sample order %.3f s, epochs %.3f s, per-epoch checks %.3f s, per-lambda deviance + rescale %.3f s\n",
            t.rng, t.run, t.chk, t.dev);
  pt.mark("lambda path (SAGA + deviance)");
  out->npasses = n_iter;
  out->draws_used = so.draws.pos;
  return close_sample_order(ranks, so, n);
}

// Runs body(X) with x's device setup and its stream in place: X.dev and X.st are set for the call and gone after it
template <class F>
int with_device_setup(const sgdnet_control* ctl, Features& X, F body) {
  const int rc_dev = check_device(ctl->device);
  if (rc_dev) return rc_dev;
  SGD_HIP_TRY(hipSetDevice(ctl->device));
  DeviceSetup dev;
  hipStream_t st = nullptr;
  SGD_HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  X.dev = &dev;
  X.st = st;
  const int rc = body(dev, st);
  dev.release();
  (void)hipStreamDestroy(st);
  return rc;
}

int fit_dense_impl(const double* x, int64_t n, int64_t p, const double* y, int y_cols, const sgdnet_control* ctl, sgdnet_result* out,
                   bool* batched_gave_up);

int fit_sparse_impl(const sgdnet_csc* x, const double* y, int y_cols, const sgdnet_control* ctl, sgdnet_result* out,
                    bool* batched_gave_up) {
  int rc = validate(ctl, out, y_cols);
  if (rc) return rc;
  if (!x || !y || x->n_rows <= 0 || x->n_cols <= 0 || !x->colptr || !x->rowidx || !x->values) {
    set_error("sgdnet_fit_sparse: invalid matrix");
    return SGDNET_EINVAL;
  }
  Features X;
  X.sparse = true;
  X.n = x->n_rows;
  X.p = x->n_cols;
  X.colptr = x->colptr;
  X.rowidx = x->rowidx;
  X.raw_values = x->values;
  const int64_t n = X.n, p = X.p, nnz = x->colptr[p];
  if ((rc = validate_colptr(x)) || (rc = validate_response(ctl, y, n)) || (rc = validate_rowidx(x))) return rc;
  if (ctl->mode == SGDNET_MODE_MNEWTON || ctl->mode == SGDNET_MODE_WNEWTON || ctl->mode == SGDNET_MODE_WMNEWTON) {
    // These modes read x dense (mnewton holds at most 98 features; wnewton's sparse moments would be p (p + 2) workgroups a
    // step; wmnewton's class-pair moments have no sparse form).  The copy is made here, before anything is computed from x, so that the standard deviations, lambda_max and
    // everything after them are the dense fit's of the same matrix, bit for bit.  The plan's refusals come first: one of
    // them is the size of this copy.  Entries stored twice add up.
    FitFacts facts;
    facts.ctl = ctl;
    facts.sparse = true;
    facts.n = n;
    facts.p = p;
    const FitPlan plan = plan_fit(facts);
    if (plan.rc) {
      set_error("%s", plan.error.c_str());
      return plan.rc;
    }
    std::vector<double> xd((size_t)(n * p), 0.0);
    for (int64_t j = 0; j < p; ++j)
      for (int64_t q = x->colptr[j]; q < x->colptr[j + 1]; ++q) xd[(size_t)(x->rowidx[q] + j * n)] += x->values[q];
    return fit_dense_impl(xd.data(), n, p, y, y_cols, ctl, out, batched_gave_up);
  }
  if (!option(kOptHostSetup) && !(ctl->n_gpus > 1)) {   // (a fit sharded over several GPUs cuts the host copy into the ranks' ranges)
    // default: the per-fit O(nnz) passes run on the device (setup_device.hip)
    return with_device_setup(ctl, X, [&](DeviceSetup& dev, hipStream_t st) {
      const int r = device_setup_begin(dev, x, ctl->standardize ? 1 : 0, st, X.x_center, X.x_scale, &X.dev_max_mean_sq);
      return r ? r : fit_common(X, y, y_cols, ctl, out, batched_gave_up);
    });
  }
  X.val.assign(x->values, x->values + nnz);
  X.x_center.assign((size_t)p, 0.0);
  X.x_scale.assign((size_t)p, 1.0);
  X.x_center_scaled.assign((size_t)p, 0.0);
  if (ctl->standardize) {                                     // utils.h:110-121, math.h:66-79,89-112
    for (int64_t j = 0; j < p; ++j) {
      const int64_t q0 = x->colptr[j], q1 = x->colptr[j + 1];
      double s = 0.0;
      for (int64_t q = q0; q < q1; ++q) s += X.val[(size_t)q];
      const double mean = s / (double)n;
      double var = 0.0;
      for (int64_t q = q0; q < q1; ++q) var += pow(X.val[(size_t)q] - mean, 2) / (double)n;
      var += (double)(n - (q1 - q0)) * mean * mean / (double)n;
      const double sd = (var == 0.0) ? 1.0 : sqrt(var);
      for (int64_t q = q0; q < q1; ++q) X.val[(size_t)q] /= sd;
      X.x_center[(size_t)j] = mean;
      X.x_scale[(size_t)j] = sd;
      X.x_center_scaled[(size_t)j] = mean / sd;             // sgdnet.cpp:150
    }
  }
  // AdaptiveTranspose (utils.h:276-281): counting sort into sample-major order
  X.sptr.assign((size_t)n + 1, 0);
  for (int64_t q = 0; q < nnz; ++q) X.sptr[(size_t)x->rowidx[q] + 1]++;
  for (int64_t i = 0; i < n; ++i) X.sptr[(size_t)i + 1] += X.sptr[(size_t)i];
  X.sidx.resize((size_t)nnz);
  X.sval.resize((size_t)nnz);
  {
    std::vector<int64_t> fill(X.sptr.begin(), X.sptr.end() - 1);
    for (int64_t j = 0; j < p; ++j)
      for (int64_t q = x->colptr[j]; q < x->colptr[j + 1]; ++q) {
        const int64_t dst = fill[(size_t)x->rowidx[q]]++;
        X.sidx[(size_t)dst] = (int32_t)j;
        X.sval[(size_t)dst] = X.val[(size_t)q];
      }
  }
  if (getenv("SGDNET_TRACE")) fprintf(stderr, "[sgdnet] features: standardize + transpose done\n");
  return fit_common(X, y, y_cols, ctl, out, batched_gave_up);
}

int fit_dense_impl(const double* x, int64_t n, int64_t p, const double* y, int y_cols, const sgdnet_control* ctl,
                   sgdnet_result* out, bool* batched_gave_up) {
  int rc = validate(ctl, out, y_cols);
  if (rc) return rc;
  if (!x || !y || n <= 0 || p <= 0) {
    set_error("sgdnet_fit_dense: invalid matrix");
    return SGDNET_EINVAL;
  }
  rc = validate_response(ctl, y, n);
  if (rc) return rc;
  Features X;
  X.sparse = false;
  X.n = n;
  X.p = p;
  X.raw_dense = x;
  if (n * p >= kDenseDeviceSetupElems && !option(kOptHostSetup)) {
    // large dense x: statistics, standardisation, lambda_max products, transpose and row norms on the
    // device (dense_setup_*), no host pass over the n * p doubles beyond the one upload
    return with_device_setup(ctl, X, [&](DeviceSetup& dev, hipStream_t st) {
      X.dense_dev = true;
      X.x_center_scaled.assign((size_t)p, 0.0);
      const int r = dense_setup_begin(dev, x, n, p, ctl->standardize ? 1 : 0, st, X.x_center, X.x_scale, &X.dev_max_mean_sq);
      return r ? r : fit_common(X, y, y_cols, ctl, out, batched_gave_up);
    });
  }
  X.xd.assign(x, x + n * p);
  X.x_center.assign((size_t)p, 0.0);
  X.x_scale.assign((size_t)p, 1.0);
  X.x_center_scaled.assign((size_t)p, 0.0);                   // sgdnet.cpp:151
  if (ctl->standardize) {                                     // utils.h:99-108
    col_mean_sd(X.xd.data(), n, p, X.x_center.data(), X.x_scale.data());
    standardize_cols(X.xd.data(), n, p, X.x_center.data(), X.x_scale.data());
  }
  if (!plans_direct(ctl->mode)) {     // (the direct modes read x column-major, as it came)
    X.xt.resize((size_t)(n * p));                             // utils.h:283-288
    transpose_to_sample_major(X.xd.data(), n, p, X.xt.data());
  }
  return fit_common(X, y, y_cols, ctl, out, batched_gave_up);
}

// mode = auto promises a fit: when the batched iteration gives up (non-finite coefficients even at the
// shortest window) the whole fit is run again in exact mode.  fit(control, &batched_gave_up) is fit_*_impl.
template <class F>
int with_exact_fallback(const sgdnet_control* ctl, F fit) {
  bool batched_gave_up = false;
  int rc = fit(ctl, &batched_gave_up);
  if (rc == SGDNET_EUNSUPPORTED && batched_gave_up && ctl && ctl->mode == SGDNET_MODE_AUTO) {
    if (getenv("SGDNET_TRACE")) fprintf(stderr, "[sgdnet] mode = auto: batched iteration gave up, fitting again in exact mode\n");
    sgdnet_control exact = *ctl;
    exact.mode = SGDNET_MODE_EXACT;
    exact.batch = 0;
    rc = fit(&exact, &batched_gave_up);
  }
  return rc;
}


}  // namespace

extern "C" {
int sgdnet_fit_sparse(const sgdnet_csc* x, const double* y, int y_cols, const sgdnet_control* ctl,
                      sgdnet_result* out) {
  return with_exact_fallback(ctl, [&](const sgdnet_control* c, bool* gave_up) { return fit_sparse_impl(x, y, y_cols, c, out, gave_up); });
}

int sgdnet_fit_dense(const double* x, int64_t n, int64_t p, const double* y, int y_cols,
                     const sgdnet_control* ctl, sgdnet_result* out) {
  return with_exact_fallback(ctl, [&](const sgdnet_control* c, bool* gave_up) { return fit_dense_impl(x, n, p, y, y_cols, c, out, gave_up); });
}

// ---- diagnostics (include/sgdnet_hip.h): the setup passes of a fit, run as a fit runs them, everything copied back ----

int sgdnet_setup_probe_sparse(const sgdnet_csc* x, int standardize, const double* ymap, int cols, const double* y, int y_rows,
                              int rec_align, int device, sgdnet_setup_probe* out) {
  if (!x || !out || x->n_rows <= 0 || x->n_cols <= 0 || !x->colptr || !x->rowidx || !x->values || !ymap || cols < 1 ||
      y_rows < 1 || !y || rec_align < 64 || rec_align % 64 || !out->center || !out->scale || !out->xty || !out->sptr ||
      !out->sidx || !out->sval || !out->rec || !out->ovf) {
    set_error("sgdnet_setup_probe_sparse: invalid argument");
    return SGDNET_EINVAL;
  }
  int rc;
  if ((rc = validate_colptr(x)) || (rc = validate_rowidx(x))) return rc;
  sgdnet_control ctl{};
  ctl.device = device;
  Features X;
  return with_device_setup(&ctl, X, [&](DeviceSetup& dev, hipStream_t st) {
    std::vector<double> center, scale;
    int r;
    if ((r = device_setup_begin(dev, x, standardize ? 1 : 0, st, center, scale, &out->max_mean_sq)) ||
        (r = device_xt_times(dev, ymap, cols, out->xty, st)) ||
        (r = device_setup_finish(dev, y, y_rows, standardize ? 1 : 0, rec_align, st, &out->max_sqnorm)) ||
        (r = device_gram_lmax(dev, standardize ? 1 : 0, st, &out->l_f)))
      return r;
    std::copy(center.begin(), center.end(), out->center);
    std::copy(scale.begin(), scale.end(), out->scale);
    out->rec_stride = dev.rec_stride;
    out->rec_cap = dev.rec_cap;
    out->rec_val_off = dev.rec_val_off;
    out->n_ovf = dev.n_ovf;
    const size_t rec_bytes = (size_t)dev.n * (size_t)dev.rec_stride, ovf_bytes = (size_t)dev.n_ovf * 256;
    if ((size_t)out->rec_bytes_cap < rec_bytes || (size_t)out->ovf_bytes_cap < ovf_bytes) {
      set_error("sgdnet_setup_probe_sparse: %zu record bytes and %zu overflow bytes, the capacities are %lld and %lld", rec_bytes,
                ovf_bytes, (long long)out->rec_bytes_cap, (long long)out->ovf_bytes_cap);
      return SGDNET_EINVAL;
    }
    SGD_HIP_TRY(hipMemcpy(out->sptr, dev.sptr, sizeof(int64_t) * ((size_t)dev.n + 1), hipMemcpyDeviceToHost));
    if (dev.nnz) {
      SGD_HIP_TRY(hipMemcpy(out->sidx, dev.sidx, sizeof(int32_t) * (size_t)dev.nnz, hipMemcpyDeviceToHost));
      SGD_HIP_TRY(hipMemcpy(out->sval, dev.sval, sizeof(double) * (size_t)dev.nnz, hipMemcpyDeviceToHost));
    }
    SGD_HIP_TRY(hipMemcpy(out->rec, dev.rec, rec_bytes, hipMemcpyDeviceToHost));
    if (ovf_bytes) SGD_HIP_TRY(hipMemcpy(out->ovf, dev.ovf, ovf_bytes, hipMemcpyDeviceToHost));
    return (int)SGDNET_OK;
  });
}

int sgdnet_setup_probe_dense(const double* x, int64_t n, int64_t p, int standardize, const double* ymap, int cols,
                             int64_t sample_stride, int64_t sample_m, int device, sgdnet_setup_probe* out) {
  if (!x || !out || n <= 0 || p <= 0 || !ymap || cols < 1 || !out->center || !out->scale || !out->xty || !out->xt ||
      sample_m < 0 || (sample_m > 0 && (!out->sample || sample_stride < 1 || (sample_m - 1) * sample_stride >= n))) {
    set_error("sgdnet_setup_probe_dense: invalid argument");
    return SGDNET_EINVAL;
  }
  sgdnet_control ctl{};
  ctl.device = device;
  Features X;
  return with_device_setup(&ctl, X, [&](DeviceSetup& dev, hipStream_t st) {
    std::vector<double> center, scale;
    int r;
    if ((r = dense_setup_begin(dev, x, n, p, standardize ? 1 : 0, st, center, scale, &out->max_mean_sq)) ||
        (r = dense_xt_times(dev, ymap, cols, out->xty, st)) ||
        (sample_m > 0 && (r = dense_sample_rows(dev, sample_stride, sample_m, out->sample, st))) ||
        (r = dense_setup_finish(dev, st, &out->max_sqnorm)))
      return r;
    std::copy(center.begin(), center.end(), out->center);
    std::copy(scale.begin(), scale.end(), out->scale);
    SGD_HIP_TRY(hipMemcpy(out->xt, dev.xd_t, sizeof(double) * (size_t)n * (size_t)p, hipMemcpyDeviceToHost));
    return (int)SGDNET_OK;
  });
}

}  // extern "C"
