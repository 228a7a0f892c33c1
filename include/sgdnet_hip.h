/*
 * sgdnet_hip.h -- C ABI of the MI355X (gfx950) SAGA elastic-net backend.
 *
 * Drop-in boundary for the hot path of jolars/sgdnet (paths below are relative
 * to the reference tree):
 *
 *   src/RcppExports.cpp:11-21,24-34  _sgdnet_SgdnetDense / _sgdnet_SgdnetSparse
 *   src/sgdnet.cpp:358-375           SgdnetDense / SgdnetSparse (x, y, control)
 *   R/sgdnet.R:346-366               the `control` list and the two call sites
 *
 * sgdnet_fit_dense / sgdnet_fit_sparse take exactly what those entry points
 * take (R's column-major matrix or dgCMatrix slots, the response matrix, the 14
 * control fields) and return exactly what src/sgdnet.cpp:275-284 returns.  The
 * R-side binding (a .Call shim over these two functions) is shown in
 * INTEGRATION.md and shim/sgdnet_shim.c.
 *
 * The sgdnet_solver_* functions expose the device-resident per-lambda SAGA
 * loop (reference src/saga-sparse.h:194-383, src/saga-dense.h:99-224) for the
 * benchmark harness, the parity tests and the multi-GPU driver.
 *
 * Plain pointers and sizes only; no C++ or torch types.  All functions return 0
 * on success or a negative SGDNET_E* code; sgdnet_last_error() describes the
 * most recent failure on the calling thread.  There is no CPU fallback: every
 * compute entry point fails with SGDNET_ENODEVICE when no HIP device exists.
 */
#ifndef SGDNET_HIP_H_
#define SGDNET_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: sgdnet_control carries losses_sink / losses_ctx, sgdnet_set_option exists.  3: sgdnet_auc_*_rng, the option
 * exact_row_registers, sgdnet_solver_rng_layout (additions only).  4: sgdnet_control ends with n_gpus / devices
 * (a fit sharded over the GPUs of a node), sgdnet_solver_link_peers, the option fused_epoch.  5: sgdnet_gradient_sparse /
 * _dense (additions only).  6: SGDNET_MODE_COVARIANCE, sgdnet_covariance_max_features, later sgdnet_cv_covariance_*, SGDNET_MODE_NEWTON, sgdnet_newton_max_features and sgdnet_cv_newton_*, SGDNET_MODE_MCOVARIANCE and sgdnet_mcovariance_max_features, SGDNET_MODE_MNEWTON and sgdnet_mnewton_max_features, sgdnet_mnewton_probe, SGDNET_MODE_WCOVARIANCE, sgdnet_wcovariance_max_features and the option wcovariance_width, SGDNET_MODE_WNEWTON, sgdnet_wnewton_max_features and the option wnewton_width, SGDNET_MODE_WMCOVARIANCE, sgdnet_wmcovariance_max_features and the option wmcovariance_width, sgdnet_cv_mnewton_*, sgdnet_cv_wcovariance_*, sgdnet_cv_wmcovariance_*, sgdnet_cv_wnewton_* (additions only).  A caller compiled against
 * another version must not pass its structs: the shim and the Python binding compare sgdnet_abi_version()
 * with this constant when they load the library. */
#define SGDNET_ABI_VERSION 6

/* error codes */
#define SGDNET_OK          0
#define SGDNET_EINVAL     -1   /* bad argument */
#define SGDNET_ENODEVICE  -2   /* no HIP device / HIP runtime failure at init */
#define SGDNET_EHIP       -3   /* HIP call failed */
#define SGDNET_ENOMEM     -4
#define SGDNET_EUNSUPPORTED -5 /* valid request outside what a mode implements */
#define SGDNET_ESTREAM    -6   /* explicit sample stream exhausted */

/* control$family (R/sgdnet.R:185-188; src/sgdnet.cpp:305-331) */
#define SGDNET_GAUSSIAN    0
#define SGDNET_BINOMIAL    1
#define SGDNET_MULTINOMIAL 2
#define SGDNET_MGAUSSIAN   3

/* penalty functor chosen by RunSaga (src/sgdnet.cpp:80-98; src/penalties.h) */
#define SGDNET_RIDGE       0
#define SGDNET_ELASTICNET  1
#define SGDNET_GROUPLASSO  2

/* execution mode of the SAGA loop */
#define SGDNET_MODE_EXACT   0  /* the reference iteration, one draw at a time, in stream order */
#define SGDNET_MODE_BATCHED 1  /* `batch` consecutive draws against one snapshot (sparse x: up to 64 classes;
                                  dense x: up to 16 classes, 17..64 through the sparse form with every entry stored); sgdnet_fit_*
                                  fall back to the exact iteration outside that */
#define SGDNET_MODE_AUTO    2  /* sgdnet_fit_* only: batched wherever it is implemented (see above), exact otherwise.  Same optimum, not the reference's
                                  iteration order; SGDNET_MODE_EXACT stays the default. */
/* sgdnet_fit_* only, and only when asked for (no other mode resolves to it): the gaussian path of one response solved
 * to its optimum from the centred cross-products X'X and X'y, which one pass over x leaves on the device; cyclic
 * coordinate descent on that p x p problem in one workgroup (sgdnet_amd/csrc/covariance.hip).  Needs family =
 * gaussian, n_classes = 1, n_features <= sgdnet_covariance_max_features(), n_gpus <= 1 and debug = 0; anything else
 * returns SGDNET_EUNSUPPORTED and sgdnet_last_error() names the condition -- there is no fall back to SAGA.
 * The fit draws no samples: sample_stream, unif, seed and rng_state are accepted and ignored, rng_state is left
 * untouched bit for bit and result.draws_used = 0.  result.npasses = the coordinate sweeps summed over the path,
 * max_iter bounds the sweeps of one lambda, tol is the reference's ConvergenceCheck applied per sweep
 * (max|dw| / max|w| <= tol), and return_codes[l] = 1 when lambda l used all max_iter sweeps without meeting tol.
 * lambda, nulldev, dev_ratio, intercept = 0 and standardize = 0 are defined as in the other modes. */
#define SGDNET_MODE_COVARIANCE 3
/* sgdnet_fit_* only, and only when asked for (no other mode resolves to it; an addition of ABI 6): the binomial path of
 * one response solved to its optimum by proximal Newton steps (IRLS).  An outer step is one pass over x that leaves
 * mu_i, v_i = mu_i (1 - mu_i) and the mean loss at the iterate, one pass that leaves the weighted Gram matrix
 * H = Z'VZ / n of the centred features and the column of ones and the gradient q = Z'(y - mu) / n, and cyclic
 * coordinate descent on the penalised quadratic model in one wavefront, the intercept an unpenalised last
 * coordinate (sgdnet_amd/csrc/newton.hip).  A step after which the penalised objective rose is halved.  Needs family =
 * binomial, n_features <= sgdnet_newton_max_features(), n_gpus <= 1 and debug = 0; anything else returns
 * SGDNET_EUNSUPPORTED and sgdnet_last_error() names the condition ("mode = newton needs ...") -- no fall back to SAGA.
 * The fit draws no samples: sample_stream, unif, seed and rng_state are accepted and ignored, rng_state is left
 * untouched bit for bit and result.draws_used = 0.  lambda is done when an outer step moves the coefficients and the
 * intercept by max|du| / max|u| <= tol (all zero counts as converged); max_iter bounds the outer steps of one lambda
 * and return_codes[l] = 1 when lambda l used them all; result.npasses = the passes over x that evaluated an iterate,
 * summed over the path.  lambda, nulldev, dev_ratio, intercept = 0 and standardize = 0 are defined as in the other
 * modes. */
#define SGDNET_MODE_NEWTON 4
/* sgdnet_fit_* only, and only when asked for (no other mode resolves to it; an addition of ABI 6): the mgaussian path of
 * n_classes responses solved to its optimum from the centred cross-products X'X and X'Y, which one pass over x leaves
 * on the device: the group lasso over the responses of a feature with its l2 part (the ridge functor at
 * elasticnet_mix = 0), by cyclic block coordinate descent in one workgroup, one Gram matrix serving all responses
 * (sgdnet_amd/csrc/covariance.hip: cov_group_path_kernel).  For 0 < elasticnet_mix < 1 this is the only mode with an
 * optimum to return: the reference's group-lasso step has no fixed point there.  Needs family =
 * mgaussian, n_features <= sgdnet_mcovariance_max_features(n_classes), n_gpus <= 1 and debug = 0; anything else returns
 * SGDNET_EUNSUPPORTED and sgdnet_last_error() names the condition ("mode = mcovariance needs ...") -- no fall back to
 * SAGA.  The fit draws no samples: sample_stream, unif, seed and rng_state are accepted and ignored, rng_state is left
 * untouched bit for bit and result.draws_used = 0.  result.npasses = the block sweeps summed over the path, max_iter
 * bounds the sweeps of one lambda, tol is the reference's ConvergenceCheck over all n_features x n_classes coefficients
 * per sweep, and return_codes[l] = 1 when lambda l used all max_iter sweeps without meeting tol.  lambda, nulldev,
 * dev_ratio, standardize_response, intercept = 0 and standardize = 0 are defined as in the other modes. */
#define SGDNET_MODE_MCOVARIANCE 5
/* sgdnet_fit_* only, and only when asked for (no other mode resolves to it; an addition of ABI 6): the multinomial path
 * of n_classes classes solved to its optimum by proximal Newton steps on the JOINT Hessian of all n_classes x
 * (n_features + 1) coordinates.  An outer step is one pass over x that leaves the class probabilities mu_ik and the
 * mean loss at the iterate, one pass that leaves the n_classes (n_classes + 1) / 2 weighted Gram matrices
 * H_kl = Z'diag(mu_k (delta_kl - mu_l)) Z / n of the centred features and the column of ones with the gradients
 * q_k = Z'(y_k - mu_k) / n, and cyclic coordinate descent on the penalised quadratic model in one workgroup, the
 * intercepts unpenalised coordinates (sgdnet_amd/csrc/mnewton.hip).  A step after which the penalised objective rose is
 * halved.  Sparse x is expanded to a dense copy first.  Needs family = multinomial with the ungrouped penalty,
 * 2 <= n_classes <= 99, n_features <= sgdnet_mnewton_max_features(n_classes), n_gpus <= 1, debug = 0 and, for sparse x,
 * n_samples x n_features x 8 bytes <= 1 GiB; anything else returns SGDNET_EUNSUPPORTED and sgdnet_last_error() names
 * the condition ("mode = mnewton needs ...") -- no fall back to SAGA.  The fit draws no samples: sample_stream, unif,
 * seed and rng_state are accepted and ignored, rng_state is left untouched bit for bit and result.draws_used = 0.
 * Stopping, max_iter, return_codes and npasses are SGDNET_MODE_NEWTON's, the change taken over all coordinates.  The
 * loss does not see a shift common to all intercepts: a0 comes back with its class mean removed.  At elasticnet_mix = 1
 * and an even n_classes the optimum need not be unique in the coefficients (its deviance and its optimality
 * conditions are).  lambda, nulldev, dev_ratio, intercept = 0 and standardize = 0 are defined as in the other modes. */
#define SGDNET_MODE_MNEWTON 6
/* sgdnet_fit_* only, and only when asked for (no other mode resolves to it; an addition of ABI 6): SGDNET_MODE_COVARIANCE's
 * problem and method for up to sgdnet_wcovariance_max_features() features.  The scaled Gram matrix stays in global memory
 * as a full symmetric matrix; one workgroup keeps c~, the coefficients, the gradient, diag S and an ascending list of the
 * coordinates that can move in its LDS, runs cyclic coordinate descent over that list and reads one column of S per
 * coordinate that moves; coordinates outside the list are screened with the full gradient and join when they would move
 * (sgdnet_amd/csrc/covariance.hip: cov_wide_path_kernel).  Takes every n_features from 1 to the limit.  Needs family =
 * gaussian, n_classes = 1, n_features <= sgdnet_wcovariance_max_features(), n_gpus <= 1 and debug = 0; anything else
 * returns SGDNET_EUNSUPPORTED and sgdnet_last_error() names the condition ("mode = wcovariance needs ...") -- no fall
 * back to SAGA or to SGDNET_MODE_COVARIANCE.  Draws, rng_state, draws_used, tol, return_codes, lambda, nulldev,
 * dev_ratio, intercept = 0 and standardize = 0 are SGDNET_MODE_COVARIANCE's; max_iter bounds the sweeps over the list
 * of one lambda and result.npasses counts those sweeps.  Same optimum as SGDNET_MODE_COVARIANCE, not the same bits. */
#define SGDNET_MODE_WCOVARIANCE 7
/* sgdnet_fit_* only, and only when asked for (no other mode resolves to it; an addition of ABI 6): SGDNET_MODE_NEWTON's
 * problem and outer loop for up to sgdnet_wnewton_max_features() features.  Per Newton step the scaled weighted Gram
 * matrix is written to global memory as a full symmetric matrix; one workgroup keeps the gradient, the coordinates,
 * diag H and an ascending list of the coordinates that can move in its LDS, runs cyclic coordinate descent over that
 * list and reads one column of H per coordinate that moves; coordinates outside the list are screened with the full
 * gradient and join when they would move; the intercept is an unpenalised member of the list
 * (sgdnet_amd/csrc/newton.hip: newton_wide_cd_kernel).  Takes every n_features from 1 to the limit.  Sparse x is
 * expanded to a dense copy (at most 1 GiB) and gives the dense fit's bits.  Needs family = binomial, n_classes = 1,
 * n_features <= sgdnet_wnewton_max_features(), n_gpus <= 1, debug = 0 and that copy within its bound; anything else
 * returns SGDNET_EUNSUPPORTED and sgdnet_last_error() names the condition ("mode = wnewton needs ...") -- no fall back
 * to SAGA or to SGDNET_MODE_NEWTON.  Draws, rng_state, draws_used, max_iter, tol, return_codes, npasses, lambda, nulldev,
 * dev_ratio, intercept = 0 and standardize = 0 are SGDNET_MODE_NEWTON's.  Same optimum as SGDNET_MODE_NEWTON, not the
 * same bits. */
#define SGDNET_MODE_WNEWTON 8
/* sgdnet_fit_* only, and only when asked for (no other mode resolves to it; an addition of ABI 6): SGDNET_MODE_MCOVARIANCE's
 * problem and method for up to sgdnet_wmcovariance_max_features(n_classes) features.  The scaled Gram matrix stays in
 * global memory as a full symmetric matrix; one workgroup keeps the coefficients and the gradient of all responses,
 * diag S and an ascending list of the blocks (a feature's n_classes coefficients) that can move in its LDS, runs cyclic
 * block coordinate descent over that list and reads one column of S per block that moves, for all responses at once;
 * blocks outside the list are screened with the full gradient and join when they would move
 * (sgdnet_amd/csrc/covariance.hip: cov_wide_group_path_kernel).  Takes every n_features from 1 to the limit; sparse x is
 * read as it is.  Needs family = mgaussian, n_features <= sgdnet_wmcovariance_max_features(n_classes), n_gpus <= 1 and
 * debug = 0; anything else returns SGDNET_EUNSUPPORTED and sgdnet_last_error() names the condition ("mode = wmcovariance
 * needs ...") -- no fall back to SAGA or to SGDNET_MODE_MCOVARIANCE.  Draws, rng_state, draws_used, tol, return_codes,
 * lambda, nulldev, dev_ratio, standardize_response, intercept = 0 and standardize = 0 are SGDNET_MODE_MCOVARIANCE's;
 * max_iter bounds the sweeps over the list of one lambda and result.npasses counts those sweeps.  Same optimum as
 * SGDNET_MODE_MCOVARIANCE, not the same bits. */
#define SGDNET_MODE_WMCOVARIANCE 9
/* sgdnet_fit_* only, and only when asked for (no other mode resolves to it; an addition of ABI 6): SGDNET_MODE_MNEWTON's
 * problem and outer loop for up to sgdnet_wmnewton_max_features(n_classes) features.  Per Newton step the scaled joint
 * Hessian of all Q = n_classes x (n_features + 1) coordinates is written to global memory as a full symmetric matrix;
 * one workgroup keeps the gradient, the coordinates, diag H and an ascending list of the coordinates that can move in
 * its LDS, runs cyclic coordinate descent over that list and reads one column of H per coordinate that moves;
 * coordinates outside the list are screened with the full gradient and join when they would move; the n_classes
 * intercepts are unpenalised members of the list (sgdnet_amd/csrc/mnewton.hip: mnewton_wide_cd_kernel).  Takes every
 * n_features from 1 to the limit.  Sparse x is expanded to a dense copy (at most 1 GiB) and gives the dense fit's bits.
 * Needs family = multinomial with the ungrouped penalty, 2 <= n_classes <= 99, n_features <=
 * sgdnet_wmnewton_max_features(n_classes), n_gpus <= 1, debug = 0 and that copy within its bound; anything else returns
 * SGDNET_EUNSUPPORTED and sgdnet_last_error() names the condition ("mode = wmnewton needs ...") -- no fall back to SAGA
 * or to SGDNET_MODE_MNEWTON.  Draws, rng_state, draws_used, max_iter, tol, return_codes, npasses, the class-centred a0,
 * lambda, nulldev, dev_ratio, intercept = 0 and standardize = 0 are SGDNET_MODE_MNEWTON's.  Same optimum as
 * SGDNET_MODE_MNEWTON, not the same bits. */
#define SGDNET_MODE_WMNEWTON 10

/* x as R passes it to SgdnetSparse: the slots of a dgCMatrix (R/sgdnet.R:226). */
typedef struct sgdnet_csc {
  int64_t        n_rows;   /* Dim[0] = samples  */
  int64_t        n_cols;   /* Dim[1] = features */
  const int32_t* colptr;   /* @p, n_cols + 1    */
  const int32_t* rowidx;   /* @i, 0-based, ascending within a column */
  const double*  values;   /* @x                */
} sgdnet_csc;

/* One uniform(0,1) draw; the R shim passes unif_rand() so that R's own RNG is
 * advanced exactly as Rcpp::RNGScope + R::runif would (src/RcppExports.cpp:14,
 * src/saga-sparse.h:261). */
typedef double (*sgdnet_unif_fn)(void* ctx);

/* Receiver of the per-epoch debug losses of one lambda (control.debug, options(sgdnet.debug = TRUE),
 * src/saga-sparse.h:350-365 / src/utils.h:199-227): called once per lambda, on the calling thread,
 * when that lambda's SAGA loop has ended, with the EpochLoss value of every epoch it ran.  The
 * reference grows a std::vector (src/saga-sparse.h:364); a sink lets the caller do the same instead
 * of reserving n_lambda x max_iter doubles (80 GB per path at the reference's benchmark setting
 * maxit = 1e8, data-raw/benchmarks.R). */
typedef void (*sgdnet_losses_fn)(void* ctx, int lambda_index, const double* losses, int count);

/* State of R's default generator (Mersenne-Twister): 625 words = mti + mt[624]. */
typedef struct sgdnet_rng { uint32_t mti; uint32_t mt[624]; } sgdnet_rng;

typedef struct sgdnet_control {
  /* ---- the control list of R/sgdnet.R:346-359, field for field ---- */
  int           debug;
  double        elasticnet_mix;
  int           family;               /* SGDNET_GAUSSIAN ... */
  int           intercept;
  int           is_sparse;            /* unused natively, as in the reference */
  const double* lambda;               /* NULL / n_lambda_user == 0 => automatic path */
  int           n_lambda_user;        /* length(control$lambda) */
  double        lambda_min_ratio;
  unsigned      max_iter;
  int           n_lambda;
  int           n_classes;
  int           standardize;
  int           standardize_response;
  double        tol;
  int           type_multinomial;     /* 0 = "ungrouped" (the only value R sends), 1 = "grouped" */

  /* ---- sample order (exactly one draw per inner iteration) ---- */
  const uint32_t* sample_stream;      /* explicit indices in [0, n), or NULL */
  int64_t         sample_stream_len;
  sgdnet_unif_fn  unif;               /* used when sample_stream == NULL and unif != NULL */
  void*           unif_ctx;
  uint32_t        seed;               /* else: built-in R-compatible Mersenne-Twister, set.seed(seed) */
  struct sgdnet_rng* rng_state;       /* else-branch only: if non-NULL the generator starts from this
                                         state (R's .Random.seed: mti + mt[624]) instead of `seed`
                                         and the advanced state is written back */

  /* ---- backend extensions; zero-initialised == reference behaviour ---- */
  int           mode;                 /* SGDNET_MODE_* */
  int64_t       batch;                /* batched mode: staleness window; 0 = automatic */
  int           device;               /* HIP device ordinal */
  sgdnet_losses_fn losses_sink;       /* debug: receives each lambda's losses (result.losses may then be NULL) */
  void*         losses_ctx;
  /* ---- ABI 4: the fit sharded over several GPUs of one node (R: options(sgdnet.gpus = N)) ----
   * n_gpus <= 1: one GPU, `device`.  n_gpus = 2..8: the samples are cut into n_gpus contiguous ranges, one solver per
   * GPU (`devices[0 .. n_gpus)`, or device, device + 1, ... when devices is NULL), each with its own virtual shards;
   * all replicas are averaged periodically inside the GPUs' epoch kernels by direct peer loads
   * (sgdnet_solver_link_peers).  Batched iteration (mode = batched / auto) of sparse x with one response, the
   * built-in generator, an even number of features; anything else returns SGDNET_EUNSUPPORTED.  The same device may
   * be named more than once (the ranks then share its CUs: rehearsals on one GPU). */
  int           n_gpus;
  const int*    devices;
} sgdnet_control;

/* Caller-allocated mirror of the list returned by src/sgdnet.cpp:275-284. */
typedef struct sgdnet_result {
  double*  a0;            /* n_classes * n_lambda            (list of numeric(K))        */
  double*  beta;          /* n_classes * n_features * n_lambda (K fastest, as unlist())  */
  double*  lambda;        /* n_lambda                                                    */
  double*  dev_ratio;     /* n_lambda                                                    */
  double*  return_codes;  /* n_lambda, 0 converged / 1 max_iter reached                  */
  double*  losses;        /* n_lambda * max_iter or NULL; filled when control.debug (or use
                             control.losses_sink, which needs no max_iter-sized block)   */
  int32_t* losses_len;    /* n_lambda or NULL                                            */
  double   nulldev;
  double   npasses;
  int64_t  draws_used;    /* inner iterations executed == uniform draws consumed         */
} sgdnet_result;

int sgdnet_abi_version(void);
const char* sgdnet_last_error(void);
int sgdnet_device_count(void);
/* the largest n_features SGDNET_MODE_COVARIANCE takes (198: what one gfx950 workgroup's LDS holds; at least 64) */
int sgdnet_covariance_max_features(void);
/* the largest n_features SGDNET_MODE_WCOVARIANCE takes (4531: 4 p doubles, p list words and p bits in one workgroup's
 * LDS; at least 4096) */
int sgdnet_wcovariance_max_features(void);
/* the largest n_features SGDNET_MODE_NEWTON takes (198: the intercept is one more coordinate of the LDS-resident model) */
int sgdnet_newton_max_features(void);
/* the largest n_features SGDNET_MODE_WNEWTON takes (5819: with the intercept 3 P doubles, P list words and P bits in one
 * workgroup's LDS, P = n_features + 1; at least 4096) */
int sgdnet_wnewton_max_features(void);
/* the largest n_features SGDNET_MODE_MCOVARIANCE takes with n_responses responses: the LDS holds p (p + 1) / 2 + 3 p K
 * doubles (195 at K = 2, 174 at K = 10, 63 at K = 96); 0 where nothing fits or n_responses < 1 */
int sgdnet_mcovariance_max_features(int n_responses);
/* the largest n_features SGDNET_MODE_WMCOVARIANCE takes with n_responses responses: the LDS holds 2 K doubles per feature
 * (the feature count rounded up to even), diag S, K doubles of scratch, p list words and p bits, and the moments pass
 * takes n_features + n_responses <= sgdnet_wcovariance_max_features() + 1 columns (4531 at K = 1, 3709 at K = 2, 2722 at
 * K = 3, 950 at K = 10, 104 at K = 96; at least 2048 at K = 2 and 512 at K = 10); 0 where nothing fits or n_responses < 1 */
int sgdnet_wmcovariance_max_features(int n_responses);
/* the largest n_features SGDNET_MODE_MNEWTON takes with n_classes classes: the LDS holds Q (Q + 1) / 2 + 2 Q doubles,
 * Q = n_classes (n_features + 1) <= 199: 199 / n_classes - 1 (98 at K = 2, 65 at K = 3, 38 at K = 5, 18 at K = 10,
 * 1 at K = 99); 0 for n_classes < 2 or >= 100 */
int sgdnet_mnewton_max_features(int n_classes);
/* the largest n_features SGDNET_MODE_WMNEWTON takes with n_classes classes: the LDS holds 3 Q doubles, Q list words and
 * Q bits, Q = n_classes (n_features + 1) <= 5820: 5820 / n_classes - 1 (2909 at K = 2, 1939 at K = 3, 1163 at K = 5,
 * 581 at K = 10, 57 at K = 99); 0 for n_classes < 2 or >= 100 */
int sgdnet_wmnewton_max_features(int n_classes);

/* ------------------------------------------------------------------------ */
/* Process-wide backend options.  These are the ONLY switches that change    */
/* how sgdnet_fit_* runs a fit; the library reads no environment variable    */
/* for that (SGDNET_TRACE prints progress to stderr and changes nothing;     */
/* kernel A/B switches exist only in -DSGDNET_EXPERIMENTS builds).           */
/*   "virtual_shards"     -1 (default): the driver's rule -- batched fits of */
/*                        up to 16 classes or responses with                 */
/*                        >= 200 000 samples run as up to 8 averaged         */
/*                        replicas; 0 or 1: never;             */
/*                        2..8: that many wherever the kernels allow it      */
/*   "rng_generators"     0 (default): 8..32 generators side by side on R's  */
/*                        one stream for epochs of >= 200 000 draws, else 1; */
/*                        1..64: that many                                   */
/*   "window_eigenvalue"  1 (default): the automatic window of sparse x uses */
/*                        the largest eigenvalue of X'X/n (power iteration); */
/*                        0: its diagonal bound only                         */
/*   "host_setup"         0 (default): standardisation, lambda_max, transpose*/
/*                        and packing run on the device for sparse x and for */
/*                        dense x of >= 4e6 elements; 1: host loops          */
/*   "exact_epoch_blocks" 1 (default): exact mode with the built-in generator*/
/*                        runs several epochs per launch; 0: one per launch  */
/*   "exact_row_registers" 1 (default): exact mode on sparse x with one      */
/*                        response and explicit x keeps the drawn row's      */
/*                        coefficients in registers for the whole draw and   */
/*                        requests the next draw's a draw ahead (same bits,  */
/*                        DESIGN.md 4.1), with several consumer wavefronts   */
/*                        where draws seldom share a feature (several classes:*/
/*                        the general iteration on eight wavefronts); 0: the general */
/*                        kernel; 2: one consumer, state kept in memory; 3:  */
/*                        several consumers wherever that is legal; 4: one   */
/*                        consumer always                                    */
/*   "fused_epoch"        1 (default): a batched epoch on virtual shards      */
/*                        (sparse x, one response) is ONE launch whose        */
/*                        workgroups synchronise shard by shard (a shard whose */
/*                        workgroups share an XCD hands off through its L2);  */
/*                        2: the same with write-through hand-offs always; 0: one */
/*                        gather and one sweep launch per batch (what the     */
/*                        library falls back to by itself when the GPU is     */
/*                        shared and the launch cannot become resident)       */
/*   "wcovariance_width"  0 (default): SGDNET_MODE_WCOVARIANCE's path kernel   */
/*                        runs on 256 or 1024 lanes by the library's rule;    */
/*                        256 or 1024: on that many (same bits either way;    */
/*                        any other value makes such a fit return             */
/*                        SGDNET_EINVAL)                                      */
/*   "wnewton_width"      0 (default): SGDNET_MODE_WNEWTON's inner solve runs  */
/*                        on 256 or 1024 lanes by the library's rule; 256 or  */
/*                        1024: on that many (same bits either way; any       */
/*                        other value makes such a fit return SGDNET_EINVAL)  */
/*   "wmcovariance_width" 0 (default): SGDNET_MODE_WMCOVARIANCE's path kernel  */
/*                        runs on 256 or 1024 lanes by the library's rule;    */
/*                        256 or 1024: on that many (same bits either way;    */
/*                        any other value makes such a fit return             */
/*                        SGDNET_EINVAL)                                      */
/*   "wmnewton_width"     0 (default): SGDNET_MODE_WMNEWTON's inner solve runs */
/*                        on 256 or 1024 lanes by the library's rule; 256 or  */
/*                        1024: on that many (same bits either way; any       */
/*                        other value makes such a fit return SGDNET_EINVAL)  */
/* Unknown names and out-of-range values return SGDNET_EINVAL.  Options are  */
/* read when a fit starts (exact_row_registers and fused_epoch: whenever     */
/* sgdnet_solver_run / _enqueue_epochs is called, i.e. once per epoch block  */
/* of a fit; the results do not depend on either); change them between fits. */
/* ------------------------------------------------------------------------ */
int sgdnet_set_option(const char* name, int value);
int sgdnet_get_option(const char* name, int* value);

/* replaces _sgdnet_SgdnetSparse (src/RcppExports.cpp:24-34 -> src/sgdnet.cpp:369-375) */
int sgdnet_fit_sparse(const sgdnet_csc* x, const double* y, int y_cols,
                      const sgdnet_control* control, sgdnet_result* out);

/* replaces _sgdnet_SgdnetDense (src/RcppExports.cpp:11-21 -> src/sgdnet.cpp:359-365);
 * x is n_samples x n_features column-major (an R numeric matrix). */
int sgdnet_fit_dense(const double* x, int64_t n_samples, int64_t n_features,
                     const double* y, int y_cols,
                     const sgdnet_control* control, sgdnet_result* out);

/* ------------------------------------------------------------------------ */
/* Built-in R-compatible Mersenne-Twister (the generator behind R::runif at  */
/* src/saga-sparse.h:261 under R's default RNGkind): 625 words = mti + mt[]. */
/* ------------------------------------------------------------------------ */
void     sgdnet_rng_seed(sgdnet_rng* r, uint32_t seed);           /* set.seed(seed)        */
double   sgdnet_rng_unif(sgdnet_rng* r);                          /* unif_rand()           */
/* Jump-ahead on the same stream (sgdnet_amd/csrc/mt_jump.cpp): poly624 <- x^draws mod phi(x), the
 * GF(2) polynomial that moves a generator state `draws` unif_rand() calls down R's stream; and its
 * application on the host.  The fit driver uses the device form to run several generators on ONE
 * set.seed() stream.  sgdnet_rng_jump_poly returns SGDNET_OK or SGDNET_EUNSUPPORTED. */
int      sgdnet_rng_jump_poly(uint64_t draws, uint32_t* poly624);
void     sgdnet_rng_jump(const sgdnet_rng* in, const uint32_t* poly624, sgdnet_rng* out);
void     sgdnet_rng_fill(sgdnet_rng* r, uint32_t n_samples,       /* floor(runif(0, n))    */
                         uint32_t* out, int64_t count);

/* ------------------------------------------------------------------------ */
/* Device-resident SAGA solver: state (w, intercept, g_memory, g_sum,        */
/* g_sum_intercept) persists across calls, i.e. across the lambda path       */
/* (src/sgdnet.cpp:187-198, 217-244).                                        */
/* ------------------------------------------------------------------------ */
typedef struct sgdnet_solver sgdnet_solver;

typedef struct sgdnet_problem {
  int      family;
  int      n_classes;        /* K */
  int64_t  n_samples;        /* samples resident on this device */
  int64_t  n_total;          /* samples of the whole job (1/n of the gradient average); 0 => n_samples */
  int64_t  n_features;
  int      fit_intercept;
  int      standardize;      /* sparse: implicit centring with x_center_scaled */
  /* sample-major data, i.e. the matrix after AdaptiveTranspose (src/sgdnet.cpp:177):
   * sparse: column i = sample i (rowptr n+1, feature ids ascending, values);
   * dense:  x_dense is n_features x n_samples column-major. */
  const int64_t* rowptr;
  const int32_t* colidx;
  const double*  values;
  const double*  x_dense;
  const double*  x_center_scaled;  /* n_features or NULL */
  const double*  y;                /* y_rows x n_samples column-major (src/sgdnet.cpp:178) */
  int            y_rows;
  int            device;
} sgdnet_problem;

int  sgdnet_solver_create(const sgdnet_problem* prob, sgdnet_solver** out);
void sgdnet_solver_destroy(sgdnet_solver* s);

/* Saga(...) arguments that change per lambda: penalty functor, step size gamma,
 * L2 strength alpha, L1 strength beta (src/saga-sparse.h:196,206-208). */
int sgdnet_solver_set_penalty(sgdnet_solver* s, int penalty, double gamma, double alpha, double beta);

/* Copy a state array between host and device.  which: 0 w (K x p), 1 intercept (K),
 * 2 g_memory (K x n), 3 g_sum (K x p), 4 g_sum_intercept (K). */
int sgdnet_solver_get_state(sgdnet_solver* s, int which, double* host);
int sgdnet_solver_set_state(sgdnet_solver* s, int which, const double* host);

/* Generate `count` sample indices floor(runif(0, n_samples)) ON THE DEVICE from the R-compatible
 * Mersenne-Twister state `rng` (replaces any previous stream); `rng` is advanced exactly as
 * sgdnet_rng_fill(rng, n_samples, out, count) would advance it. */
int sgdnet_solver_generate_stream(sgdnet_solver* s, sgdnet_rng* rng, int64_t count);

/* Copy `count` entries of the resident stream, starting at `offset`, back to the host. */
int sgdnet_solver_get_stream(sgdnet_solver* s, uint32_t* host, int64_t offset, int64_t count);

/* Make `count` sample indices resident on the device (replaces any previous stream). */
int sgdnet_solver_upload_stream(sgdnet_solver* s, const uint32_t* host, int64_t count);

/* Run the SAGA loop of one lambda on the resident stream starting at `stream_offset`:
 * epochs of `draws_per_epoch` inner iterations until ConvergenceCheck
 * (src/utils.h:240-262) passes or max_epochs is reached.  Blocks until done.
 * losses (max_epochs doubles) may be NULL. */
int sgdnet_solver_run(sgdnet_solver* s, int mode, int64_t batch,
                      int64_t stream_offset, int64_t draws_per_epoch,
                      unsigned max_epochs, double tol,
                      unsigned* epochs_run, int* converged, double* losses);

/* Enqueue `n_epochs` batched epochs without convergence checks or host
 * synchronisation (benchmark stepping).  sgdnet_solver_sync waits for them. */
int sgdnet_solver_enqueue_epochs(sgdnet_solver* s, int64_t batch, int64_t stream_offset,
                                 int64_t draws_per_epoch, int n_epochs);
int sgdnet_solver_sync(sgdnet_solver* s);

/* Sample order produced on the device, one epoch ahead of the epoch that consumes it, on a side
 * stream (what sgdnet_fit_* does for the built-in generator).  generators > 1 runs that many
 * Mersenne-Twisters side by side ON THE ONE STREAM `rng` defines (jump-ahead, see
 * sgdnet_rng_jump_poly): the draws are those of a single generator whatever the count.
 *   rng_open(s, &rng, n, G); for every epoch { rng_next(s, &off); run / enqueue an epoch with
 *   stream_offset = off; rng_done(s); }  rng_close(s, &rng) -> rng = the state after exactly the
 *   epochs that were consumed (a speculative generation is discarded).
 * With virtual shards the draws come in the layout sgdnet_solver_set_virtual_shards describes;
 * sgdnet_solver_rng_layout (before rng_open) cuts an epoch into runs of draws_per_run draws -- what a
 * sample-sharded rank does between two merges with the other ranks -- each laid out shard after
 * shard, the last one shorter if the epoch does not divide (0: one run = the epoch). */
int sgdnet_solver_rng_layout(sgdnet_solver* s, int64_t draws_per_run);
int sgdnet_solver_rng_open(sgdnet_solver* s, sgdnet_rng* rng, int64_t draws_per_epoch, int generators);
int sgdnet_solver_rng_next(sgdnet_solver* s, int64_t* stream_offset);
int sgdnet_solver_rng_done(sgdnet_solver* s);
int sgdnet_solver_rng_close(sgdnet_solver* s, sgdnet_rng* rng);

/* One batched epoch launched eagerly with HIP events around every gather
 * kernel launch; returns summed kernel time and launch count. */
int sgdnet_solver_profile_epoch(sgdnet_solver* s, int64_t batch, int64_t stream_offset,
                                int64_t draws_per_epoch, double* gather_ms, int* gather_launches,
                                double* sweep_ms, int* sweep_launches);

/* Dispatch timing of the fused epoch launches (gather form 3) enqueued from now on: enable != 0 starts collecting
 * start / stop events bound to every such launch on the solver's stream; every call first synchronises and returns
 * what was collected since the previous call (summed kernel milliseconds, launches) -- the benchmark brackets
 * exactly its timed region with two calls.  Either pointer may be NULL. */
int sgdnet_solver_epoch_timing(sgdnet_solver* s, int enable, double* sum_ms, int* launches);

/* Which gather kernel a batch of `batch` draws uses: 0 = saga_batch_gather_kernel (global
 * atomics), 1 = saga_batch_gather_lds_kernel (LDS-privatised scatter), 2 = the binned form
 * (saga_binned_gather_kernel + saga_binned_sweep_kernel: K x p tables that fit no LDS; valid after a
 * run / enqueue with that batch has sized its scratch), 3 = the fused epoch of the virtual shards
 * (saga_vs_epoch_kernel: gathers, sweeps and merges of a whole epoch in one launch). */
int sgdnet_solver_gather_form(const sgdnet_solver* s, int64_t batch);

/* Sample-sharded solvers of ONE process, one per GPU of a node: after this call the periodic
 * replica average of every solver's batched epochs runs over the virtual shards of ALL of them -- inside the
 * fused epoch kernel, by direct loads from the other GPUs' exchange buffers (hipDeviceEnablePeerAccess) behind
 * counters the ranks add to remotely; no collective library, no launch per merge.  Rank q holds a contiguous
 * range of the samples; every solver needs the same number of virtual shards, and the epochs of all ranks must be
 * enqueued (sgdnet_solver_enqueue_epochs) before any of them is waited for.  n == 1 unlinks.
 * sgdnet_fit_sparse does all of this itself when control.n_gpus > 1. */
int sgdnet_solver_link_peers(sgdnet_solver** solvers, int n);
/* The same link between solvers of DIFFERENT processes (one process per GPU): every rank fills
 * sgdnet_solver_peer_info_bytes() bytes with sgdnet_solver_peer_info (hipIpc handles of its exchange buffer and counters,
 * its shard sizes), the caller gathers the ranks' blocks in rank order (any transport: MPI, torch.distributed, a pipe) and
 * every rank calls sgdnet_solver_link_ipc with all of them; a barrier of the caller's must separate the last link from the
 * first epoch.  The peers' buffers are mapped with hipIpcOpenMemHandle and unmapped when the solver is destroyed. */
int sgdnet_solver_peer_info_bytes(void);
int sgdnet_solver_peer_info(sgdnet_solver* s, void* out);
int sgdnet_solver_link_ipc(sgdnet_solver* s, int rank, int n_ranks, const void* infos);
/* CUs a solver's batched launches may fill (0: the device's): linked solvers that share ONE GPU -- tests, or two
 * fits side by side -- must fit their persistent launches side by side. */
int sgdnet_solver_set_cu_budget(sgdnet_solver* s, int cus);

/* 2 * sum_i Loss_i (src/utils.h:304-329) over the resident samples. */
int sgdnet_solver_deviance(sgdnet_solver* s, double* out);

/* Multi-GPU merge: buffers hold 2*K*p + 2*K doubles in DEVICE memory:
 * [g_sum - g_sum_ref | w - w_ref | g_sum_intercept - ref | intercept - ref].
 * snapshot() records the reference point before a local epoch; export_delta() writes
 * the deltas; apply_merged() sets state = ref + {1, w_weight, 1, w_weight} * merged. */
int sgdnet_solver_snapshot(sgdnet_solver* s);
int sgdnet_solver_export_delta(sgdnet_solver* s, void* device_buf);
int sgdnet_solver_apply_merged(sgdnet_solver* s, const void* device_buf, double w_weight);
int64_t sgdnet_solver_delta_len(const sgdnet_solver* s);

/* The solver's HIP stream (a hipStream_t), so that a caller can order its own device work
 * -- e.g. the RCCL all-reduce of the merge buffer -- after the solver's kernels without host
 * synchronisation.  export_delta_async / apply_merged_async only enqueue. */
void* sgdnet_solver_stream(sgdnet_solver* s);
int sgdnet_solver_export_delta_async(sgdnet_solver* s, void* device_buf);
/* same, every delta multiplied by `weight` (the shard's share n_local / n_total) */
int sgdnet_solver_export_delta_weighted_async(sgdnet_solver* s, void* device_buf, double weight);
/* state <- snapshot + merged (coefficients: + w_weight * merged); the result also becomes the
 * snapshot of the next local run */
int sgdnet_solver_apply_merged_async(sgdnet_solver* s, const void* device_buf, double w_weight);

/* ------------------------------------------------------------------------ */
/* Synchronous sample-sharded batches: a global batch is split  */
/* across the ranks; every rank gathers its share into the bound buffer       */
/* [D (K*p) | intercept-accumulator slots (2*256*K)], the caller sums the     */
/* buffer across ranks on sgdnet_solver_stream() (RCCL all-reduce), then      */
/* every rank sweeps with the GLOBAL draw count.  The iterates are those of   */
/* the single-GPU batched mode with batch = that global count.                */
/* ------------------------------------------------------------------------ */
int64_t sgdnet_solver_sync_buffer_len(const sgdnet_solver* s);            /* doubles */
int sgdnet_solver_sync_bind(sgdnet_solver* s, void* device_buf);         /* NULL: unbind */
int sgdnet_solver_sync_begin(sgdnet_solver* s, int64_t stream_offset, int64_t draws_local_per_epoch);
int sgdnet_solver_sync_gather(sgdnet_solver* s, int64_t t0_local, int64_t m_local, int round);
int sgdnet_solver_sync_sweep(sgdnet_solver* s, int64_t m_global, int64_t m_local, int round);
int sgdnet_solver_sync_end(sgdnet_solver* s, int rounds);

/* Virtual shards (batched mode; one response: sparse x with or without implicit centring, or dense x;
 * 2..16 classes or responses: sparse or dense x whose n_classes x n_features table fits the LDS): the samples are
 * split into n_shards contiguous ranges (sizes as shard_bounds of sgdnet_amd/parallel.py), every
 * range runs the batched iteration on its own replica of (w, g_sum, intercept) with local
 * normalisation, one launch carries the same batch of all shards, and the replicas are averaged
 * on the device every n / 32 draws per shard.  An epoch of `draws` consumes draws / n_shards
 * stream entries per shard, laid out shard after shard: entry t of shard v of the epoch at
 * stream offset o is stream[o + v * (draws / n_shards) + t] and must be a sample of shard v.
 * sgdnet_solver_generate_stream produces that layout.  0 or 1 switches it off. */
int sgdnet_solver_set_virtual_shards(sgdnet_solver* s, int n_shards);
/* draws per shard between two device-side averages (0: n_samples / 32).  A multi-GPU job sets
 * n_total / 32 of the whole job and merges across GPUs at the same cadence. */
int sgdnet_solver_set_merge_period(sgdnet_solver* s, int64_t draws_per_shard);

/* The n that g_sum increments are divided by (default: n_total of the problem description).
 * A sample-sharded job sets it to the shard size (local normalisation) or to the
 * job's sample count (synchronous mode). */
int sgdnet_solver_set_n_total(sgdnet_solver* s, int64_t n_total);

/* ConvergenceCheck on the current w against the previous call's w (device-side). */
int sgdnet_solver_convergence(sgdnet_solver* s, double tol, int* converged);

/* max|w - w_prev| and max|w| of the most recent ConvergenceCheck (src/utils.h:248-249). */
int sgdnet_solver_last_change(const sgdnet_solver* s, double* max_change, double* max_size);

/* ---- prediction and prediction error along the lambda path ----
 * Device versions of what the reference does on the host in R: predict.sgdnet
 * (R/predict.sgdnet.R:347-402, type = "link": cbind2(1, newx) %*% beta for every lambda) and
 * score.sgdnet_<family> (R/score.R:55-186), which cv_sgdnet (R/cv_sgdnet.R:161-199) calls once per
 * (alpha, fold).  x is SAMPLE-major: CSR (rowptr int64[n+1], colidx int32, values) or dense
 * row-major n x p.  a0 is K x n_lambda and beta K x p x n_lambda, K fastest, exactly as
 * sgdnet_result holds them.  y as in sgdnet_fit_*: y_rows x n (class index for binomial /
 * multinomial).  out: one value per lambda; link: n x n_lambda x K (K fastest). */
#define SGDNET_MEASURE_DEVIANCE 0
#define SGDNET_MEASURE_MSE      1
#define SGDNET_MEASURE_MAE      2
#define SGDNET_MEASURE_CLASS    3   /* binomial / multinomial */
int sgdnet_score_sparse(int64_t n, int64_t p, const int64_t* rowptr, const int32_t* colidx, const double* values,
                        const double* y, int y_rows, int family, int n_classes, const double* a0,
                        const double* beta, int n_lambda, int measure, int device, double* out);
int sgdnet_score_dense(const double* x, int64_t n, int64_t p, const double* y, int y_rows, int family,
                       int n_classes, const double* a0, const double* beta, int n_lambda, int measure, int device,
                       double* out);
/* type.measure = "auc" of score.sgdnet_binomial (R/score.R:98-99; auc() :203-233, the weighted branch the
 * two-column indicator matrix selects).  y: class codes 0 / 1.  tie: the reference orders equal probabilities
 * by stats::runif(2n) drawn per lambda -- pass those draws, 2n per lambda (entry i for a class-0 sample i,
 * entry n + i for a class-1 sample), or NULL to break ties by position in the stacked vector (class-0 entries
 * first, then sample order).  out: one area per lambda. */
#define SGDNET_MEASURE_AUC      4   /* binomial; through sgdnet_score_*: no tie vector */
int sgdnet_auc_sparse(int64_t n, int64_t p, const int64_t* rowptr, const int32_t* colidx, const double* values,
                      const double* y, const double* a0, const double* beta, int n_lambda, const double* tie,
                      int device, double* out);
int sgdnet_auc_dense(const double* x, int64_t n, int64_t p, const double* y, const double* a0, const double* beta,
                     int n_lambda, const double* tie, int device, double* out);
/* The same with the tie breakers drawn on the device: stats::runif(2n) per lambda, in lambda order, from *rng, which
 * is left where 2 n n_lambda calls of unif_rand() leave R's generator (round 3; before, the caller drew them). */
int sgdnet_auc_sparse_rng(int64_t n, int64_t p, const int64_t* rowptr, const int32_t* colidx, const double* values,
                          const double* y, const double* a0, const double* beta, int n_lambda, sgdnet_rng* rng,
                          int device, double* out);
int sgdnet_auc_dense_rng(const double* x, int64_t n, int64_t p, const double* y, const double* a0, const double* beta,
                         int n_lambda, sgdnet_rng* rng, int device, double* out);
int sgdnet_predict_sparse(int64_t n, int64_t p, const int64_t* rowptr, const int32_t* colidx,
                          const double* values, int n_classes, const double* a0, const double* beta,
                          int n_lambda, int device, double* link);
int sgdnet_predict_dense(const double* x, int64_t n, int64_t p, int n_classes, const double* a0, const double* beta,
                         int n_lambda, int device, double* link);

/* ---- the averaged loss gradient along a fitted path (ABI 5): what an optimality (KKT) check needs from the data ----
 * G[k, j, l] = (1/n) sum_i x_ij * r_ik(l)   (K x p x n_lambda, K fastest, the layout of sgdnet_result.beta)
 * G0[k, l]   = (1/n) sum_i r_ik(l)          (K x n_lambda,     the layout of sgdnet_result.a0)
 * r_i(l) = the family's Gradient (sgdnet_amd/csrc/device_math.hpp; reference src/families.h) at the linear predictor
 * a0[:, l] + beta[:, :, l]' x_i, on the ORIGINAL x and y: no centring, no scaling, no penalty term.
 * x and y are exactly what sgdnet_fit_sparse / sgdnet_fit_dense take (dgCMatrix slots or a column-major matrix; y is
 * n x y_cols column-major, class codes for binomial / multinomial), a0 and beta as sgdnet_result holds them.
 * f64 throughout, no floating-point atomics: the same input gives the same bits (sgdnet_amd/csrc/gradient.hip).
 * SGDNET_EINVAL: null pointers, non-positive sizes, a class code outside the family's classes; SGDNET_EUNSUPPORTED:
 * more classes than sgdnet_score_* take.  sgdnet_amd/kkt.py turns (G, G0) into the optimality residual of a fit. */
int sgdnet_gradient_sparse(const sgdnet_csc* x, const double* y, int y_cols, int family, int n_classes,
                           const double* a0, const double* beta, int n_lambda, int device,
                           double* G, double* G0);
int sgdnet_gradient_dense(const double* x, int64_t n, int64_t p, const double* y, int y_cols, int family,
                          int n_classes, const double* a0, const double* beta, int n_lambda, int device,
                          double* G, double* G0);

/* Default staleness window of the batched mode: about 2 * L_max / L_F, where L_max is the
 * largest squared sample norm and L_F is bounded below by the largest mean squared feature
 * value (the diagonal of X'X/n); clamped to [64, 131072].  DESIGN.md "Choosing the batch".
 * sgdnet_fit_* apply the same rule with the largest eigenvalue of X'X/n where it is cheap (dense x: power
 * iteration, plus the constant feature), let it go down to 8 draws, and under SGDNET_MODE_AUTO take the exact
 * iteration when the rule asks for less than that or an epoch would be more than 16384 batches. */
int64_t sgdnet_auto_batch(double max_sample_sqnorm, double max_feature_mean_sq);

/* The window of a fit with virtual shards: a shard's epoch of `draws_per_shard` draws is ceil(draws_per_shard / window)
 * rounds, each with a fixed hand-off cost inside the epoch kernel.  When `window` (sgdnet_auto_batch's, capped) leaves a
 * short last round and a window at most 1/8 longer saves that round, the longer one is returned (config 4: 1 250 000 draws
 * per shard, 131 072 -> 138 889: nine rounds instead of ten); `window` otherwise.  sgdnet_fit_* apply it to their automatic
 * window (the rule of sgdnet_auto_batch keeps a factor 3 to the unstable regime; 1/8 of it is spent here). */
int64_t sgdnet_shard_window(int64_t window, int64_t draws_per_shard);

/* ------------------------------------------------------------------------ */
/* Diagnostics (additions only; the ABI version stays): what the device      */
/* setup passes of a fit (sgdnet_amd/csrc/setup_device.hip) leave behind,     */
/* copied back pass by pass.  The probes call the functions sgdnet_fit_* call,*/
/* in the order a fit calls them, on the caller's data; tests compare every   */
/* output with an exact reference (tests/test_gpu_setup_passes.py).           */
/* Every pointer is a caller-allocated HOST buffer.  The two sizes the caller */
/* cannot know in advance are capacities: rec_bytes_cap >= n * rec_stride and */
/* ovf_bytes_cap >= 256 * n_ovf, else SGDNET_EINVAL (the scalar outputs,      */
/* n_ovf among them, are filled in all the same, so a second call can size    */
/* them).  Safe upper bounds: rec_stride <= 6400 (a cap of 512 entries at     */
/* rec_align <= 256), n_ovf <= nnz / 20 + n.                                  */
/* ------------------------------------------------------------------------ */
typedef struct sgdnet_setup_probe {
  /* both probes */
  double*  center;         /* p: column means (0 without standardize)                      */
  double*  scale;          /* p: population sds, 0 -> 1 (1 without standardize)            */
  double*  xty;            /* p x cols: x' ymap of the prepared x                           */
  double   max_mean_sq;    /* max_j mean_i x_ij^2 of the prepared x (sparse: scaled, not centred) */
  double   max_sqnorm;     /* largest squared row norm of the prepared (sparse: centred) x */
  /* sparse probe: the sample-major matrix, the packed records and their geometry, L_F */
  int64_t* sptr;           /* n + 1 */
  int32_t* sidx;           /* nnz   */
  double*  sval;           /* nnz   */
  char*    rec;            /* n * rec_stride raw record bytes   */
  int64_t  rec_bytes_cap;
  char*    ovf;            /* 256 * n_ovf raw overflow bytes    */
  int64_t  ovf_bytes_cap;
  int      rec_stride, rec_cap, rec_val_off;
  int64_t  n_ovf;
  double   l_f;            /* device_gram_lmax: largest eigenvalue of X'X/n by power iteration */
  /* dense probe */
  double*  xt;             /* p x n column-major: the sample-major standardised matrix */
  double*  sample;         /* sample_m x p column-major: rows r * sample_stride, r < sample_m (NULL / 0: skipped) */
} sgdnet_setup_probe;

/* x as sgdnet_fit_sparse takes it; ymap n x cols column-major (what lambda_max multiplies by); y is y_rows x n as the
 * solvers read it (it rides in the records when y_rows == 1); rec_align: a positive multiple of 64 (a fit uses 128). */
int sgdnet_setup_probe_sparse(const sgdnet_csc* x, int standardize, const double* ymap, int cols, const double* y,
                              int y_rows, int rec_align, int device, sgdnet_setup_probe* out);
/* x n x p column-major as sgdnet_fit_dense takes it (any size: the probe does not apply the 4e6-element threshold). */
int sgdnet_setup_probe_dense(const double* x, int64_t n, int64_t p, int standardize, const double* ymap, int cols,
                             int64_t sample_stride, int64_t sample_m, int device, sgdnet_setup_probe* out);

/* Newton mode (sgdnet_amd/csrc/newton.hip), one outer step pass by pass.  The probes go through the host steps a fit
 * goes through (setup and upload, publish / blend, state pass, moments pass, inner solve): the same kernels on the same
 * grids in the same order, every output copied back; tests compare each with an exact reference
 * (tests/test_gpu_newton_passes.py).  The candidate u is published as it is (newton_blend_kernel at t = 1); the state
 * pass is taken there; the moments are those of that state; the inner solve runs on them about u_cur; last, u is
 * blended with u_cur at t.  Every pointer is a caller-allocated HOST buffer; a NULL output pointer skips that output.
 * SGDNET_EINVAL: a missing input, n or p < 1, max_sweeps = 0.  SGDNET_EUNSUPPORTED ("mode = newton needs ..."): more
 * than sgdnet_newton_max_features() features. */
typedef struct sgdnet_newton_probe {
  /* inputs */
  const double* y;         /* n: class codes 0 / 1                                                   */
  const double* scale;     /* p: the sd feature j is standardised with                               */
  const double* u_cur;     /* p + 1: the iterate (coefficients of the standardised problem, intercept) */
  const double* u;         /* p + 1: the candidate the state is taken at                             */
  double   t;              /* blend factor                                                           */
  double   l2, l1, tol;    /* the inner solve's penalty strengths and tolerance                      */
  int      centre, ridge, fit_intercept;
  unsigned max_sweeps;
  /* outputs */
  double*  mean;           /* p: cov_sum_kernel's column means (0 where centre is 0)                 */
  double*  pub_u;          /* p + 1: u after the publish at t = 1 ...                                */
  double*  pub_a;          /* p + 1: ... its state-pass form (w_j / s_j, b) ...                      */
  double   pub_rec[4];     /* ... and its record: |w|^2 / 2, |w|_1, max|u - u_cur|, max|u|            */
  double*  blend_u;        /* the same three after the blend at t                                    */
  double*  blend_a;
  double   blend_rec[4];
  double*  v;              /* n: the weights t (1 - t) of the state pass                             */
  double*  r;              /* n: its residuals y - mu                                                */
  double   loss, V, R;     /* the mean loss, sum v, sum r (newton_finish_kernel)                     */
  double*  M;              /* (p + 2)^2, row-major: entries (j, k), j <= k, of the moments of [x - m | 1 | q] (column p
                              the ones, column p + 1 q) and the corners (p, p) = V, (p, p + 1) = R; nothing else is defined */
  double*  cd_u;           /* p + 1: the inner solve's candidate ...                                 */
  double*  cd_a;           /* p + 1                                                                  */
  double   cd_rec[8];      /* ... and the whole record: loss, |w|^2 / 2, |w|_1, change, size, sweeps, converged, negligible */
} sgdnet_newton_probe;

int sgdnet_newton_probe_dense(const double* x, int64_t n, int64_t p, int device, sgdnet_newton_probe* io);
int sgdnet_newton_probe_sparse(const sgdnet_csc* x, int device, sgdnet_newton_probe* io);

/* Multinomial Newton mode (sgdnet_amd/csrc/mnewton.hip), one outer step pass by pass (additions only; the ABI version
 * stays).  Dense x only: a fit in this mode expands sparse x before anything is computed from it.  The probe goes through
 * the host steps a fit goes through (setup and upload, publish at t = 1, state pass, moments pass, inner solve, blend at
 * t): the same kernels on the same grids in the same order, every output copied back; tests compare each with an exact
 * reference (tests/test_gpu_mnewton_passes.py).  Coordinate (k, j) of u_cur, u and of every candidate lives at
 * k (p + 1) + j, j = p the intercept of class k; Q = K (p + 1).  The candidate u is published as it is; the state pass
 * is taken there; the moments are those of that state; the inner solve runs on them about u_cur; last, u is blended
 * with u_cur at t.  Every pointer is a caller-allocated HOST buffer; a NULL output pointer skips that output.
 * SGDNET_EINVAL: a missing input, n or p < 1, K < 2, max_sweeps = 0, a width other than 0 / 64 / 256.
 * SGDNET_EUNSUPPORTED ("mode = mnewton needs ..."): more than sgdnet_mnewton_max_features(K) features. */
typedef struct sgdnet_mnewton_probe_io {
  /* inputs */
  const double* y;         /* n: class codes 0 .. K - 1                                              */
  int      K;              /* classes                                                                */
  const double* scale;     /* p: the sd feature j is standardised with                               */
  const double* u_cur;     /* Q: the iterate (per class the coefficients of the standardised problem, then the intercept) */
  const double* u;         /* Q: the candidate the state is taken at                                 */
  double   t;              /* blend factor                                                           */
  double   l2, l1, tol;    /* the inner solve's penalty strengths and tolerance                      */
  int      centre, ridge, fit_intercept;
  unsigned max_sweeps;
  int      width;          /* lanes of the inner solve's workgroup: 64 or 256; 0: the rule a fit follows */
  /* outputs */
  double*  mean;           /* p: cov_sum_kernel's column means (0 where centre is 0)                 */
  double*  pub_u;          /* Q: u after the publish at t = 1 ...                                    */
  double*  pub_a;          /* Q: ... its state-pass form (w_kj / s_j, b_k) ...                       */
  double   pub_rec[4];     /* ... and its record: sum_k |w_k|^2 / 2, sum_k |w_k|_1, max|u - u_cur|, max|u| */
  double*  blend_u;        /* the same three after the blend at t                                    */
  double*  blend_a;
  double   blend_rec[4];
  double*  mu;             /* n x K, a column per class: the softmax of the state pass               */
  double   loss;           /* the mean loss (mnewton_finish_kernel)                                  */
  double*  M;              /* K (K + 1) / 2 blocks of (p + 2)^2, row-major; block c is the class pair (k, l), k <= l, in the
                              order (0, 0), (0, 1), .., (0, K - 1), (1, 1), ..  Defined in a block: entries (a, b), a <= b <= p
                              (the weighted moments of [x - m | 1], column p the ones), for every pair; entries (a, p + 1),
                              a <= p (the q column), for the pairs k = l; for the pairs k < l column p + 1 is exactly 0.0.
                              Nothing else is defined */
  double*  cd_u;           /* Q: the inner solve's candidate ...                                     */
  double*  cd_a;           /* Q                                                                      */
  double   cd_rec[8];      /* ... and the whole record: loss, |w|^2 / 2, |w|_1, change, size, sweeps, converged, negligible */
} sgdnet_mnewton_probe_io;

int sgdnet_mnewton_probe(const double* x, int64_t n, int64_t p, int device, sgdnet_mnewton_probe_io* io);

/* The wide Newton modes (SGDNET_MODE_WNEWTON, SGDNET_MODE_WMNEWTON), one outer step pass by pass (additions only; the ABI
 * version stays).  Dense x only: a wide fit expands sparse x before anything is computed from it.  The probes go through
 * the host steps a wide fit goes through (setup and upload, publish at t = 1, state pass, moments pass on the wide
 * modes' row chunks, scale kernel, list solve, blend at t): the same kernels on the same grids in the same order, every
 * output copied back; H, Hd and q are copied between the scale kernel and the solve.  Tests compare each with an exact
 * reference (tests/test_gpu_wnewton_passes.py, tests/test_gpu_wmnewton_passes.py).  The fields the narrow probes have
 * mean what they mean there; count = p + 1 (wnewton) or Q = K (p + 1) (wmnewton) coordinates.
 * SGDNET_EINVAL: a missing input, n or p < 1, K < 2, max_sweeps = 0, a width other than 0 / 256 / 1024.
 * SGDNET_EUNSUPPORTED ("mode = wnewton needs ..." / "mode = wmnewton needs ..."): more than sgdnet_wnewton_max_features()
 * / sgdnet_wmnewton_max_features(K) features.  Both are decided before any HIP call. */
typedef struct sgdnet_wnewton_probe_io {
  /* inputs (sgdnet_newton_probe) */
  const double* y;
  const double* scale;
  const double* u_cur;
  const double* u;
  double   t;
  double   l2, l1, tol;
  int      centre, ridge, fit_intercept;
  unsigned max_sweeps;
  int      width;          /* lanes of the list solve's workgroup: 256 or 1024; 0: the rule a fit follows */
  /* outputs (sgdnet_newton_probe) */
  double*  mean;
  double*  pub_u;
  double*  pub_a;
  double   pub_rec[4];
  double*  blend_u;
  double*  blend_a;
  double   blend_rec[4];
  double*  v;
  double*  r;
  double   loss, V, R;
  double*  M;
  double*  cd_u;
  double*  cd_a;
  double   cd_rec[8];
  /* outputs of the scale kernel */
  int      ld;             /* the leading dimension of H: count rounded up to a multiple of 16                 */
  double*  H;              /* ld x count, column-major as the kernel wrote it: H[k + ld j], the rows count .. ld - 1
                              (the zero pad) included                                                          */
  double*  Hd;             /* count: diag H                                                                    */
  double*  q;              /* count: the right-hand side                                                       */
} sgdnet_wnewton_probe_io;

int sgdnet_wnewton_probe(const double* x, int64_t n, int64_t p, int device, sgdnet_wnewton_probe_io* io);

typedef struct sgdnet_wmnewton_probe_io {
  /* inputs (sgdnet_mnewton_probe_io) */
  const double* y;
  int      K;
  const double* scale;
  const double* u_cur;
  const double* u;
  double   t;
  double   l2, l1, tol;
  int      centre, ridge, fit_intercept;
  unsigned max_sweeps;
  int      width;          /* lanes of the list solve's workgroup: 256 or 1024; 0: the rule a fit follows */
  /* outputs (sgdnet_mnewton_probe_io) */
  double*  mean;
  double*  pub_u;
  double*  pub_a;
  double   pub_rec[4];
  double*  blend_u;
  double*  blend_a;
  double   blend_rec[4];
  double*  mu;
  double   loss;
  double*  M;
  double*  cd_u;
  double*  cd_a;
  double   cd_rec[8];
  /* outputs of the scale kernel (sgdnet_wnewton_probe_io) */
  int      ld;
  double*  H;
  double*  Hd;
  double*  q;
} sgdnet_wmnewton_probe_io;

int sgdnet_wmnewton_probe(const double* x, int64_t n, int64_t p, int device, sgdnet_wmnewton_probe_io* io);

/* The covariance family (sgdnet_amd/csrc/covariance.hip), stage by stage.  The probes go through the host functions a fit
 * goes through (one fit: covariance_run, wcovariance_run, mcovariance_run, wmcovariance_run; a cross-validation: the stage
 * behind sgdnet_cv_*covariance_* and its covariance_cv_run, wcovariance_cv_run, mcovariance_cv_run, wmcovariance_cv_run)
 * with a tap: the same kernels on the same grids with the same arguments, and behind the stages, before the path kernel
 * is launched, device-to-host copies of what they left; then, behind the path kernel, of what it wrote.
 * tests/test_gpu_covariance_passes.py and tests/test_gpu_cv_covariance_passes.py compare each stage with an exact
 * reference, tests/test_gpu_covariance_path_passes.py and tests/test_gpu_cv_covariance_path_passes.py the path kernels.  The result is a set of named arrays of
 * doubles (int32 fields are converted), owned by the library until sgdnet_cov_probe_free.
 *
 * exactly one of x_dense (n x p column-major) and x_sparse is given.  wide = 0: the narrow form (SGDNET_MODE_COVARIANCE /
 * _MCOVARIANCE), 1: the wide form (_WCOVARIANCE / _WMCOVARIANCE).
 *
 * sgdnet_covariance_probe: y n x K column-major as the driver would hand it over (preprocessed), scale p, one mix and
 * n_lambda lambdas (the penalties (1 - mix) lambda and mix lambda; mix = 0 is the ridge functor).  multi = 0 is the
 * one-response form (K must be 1), 1 the K-response form.  SGDNET_EUNSUPPORTED, in the plan's words ("mode = covariance
 * needs no more features than sgdnet_covariance_max_features(): ..."): more features than the mode's limit.
 * SGDNET_EINVAL: a missing input, a mix outside [0, 1].  Fields, P = p + K:
 *   mu   one response: p + 2 -- the centres (0 where not centred), the response's sum, its mean.  K responses: P -- the
 *        centres and the K sums
 *   M    P x P, symmetric bit for bit.  Sparse x: the response-by-response block (rows and columns >= p) is NOT DEFINED
 *        (nothing writes it, nothing reads it)
 *   wide: ld (1); S p x ld, row j = column j of the scaled matrix, the zero pad k >= p included; Sd p; ct p x K
 *   narrow: c p x K, the path kernel's c~
 *   the path kernel's own: W, G n_lambda x p x K (the coefficients and the gradient S w - c~ of the standardised problem
 *        at the end of every lambda), sweeps, unconverged n_lambda, and tol (1), max_iter (1) as the kernel got them
 * sgdnet_covariance_path_probe: the same with the stopping rule and the path kernel's workgroup chosen.  tol and max_iter
 * (the list sweeps of one lambda) go to the kernel as they are; width = 0 is the rule a fit follows, otherwise 64 or 256
 * (multi and not wide) or 256 or 1024 (wide).  SGDNET_EINVAL, before any HIP call: any other width, max_iter = 0.
 * sgdnet_covariance_probe is this entry with tol = 1e-7, max_iter = 1000, width = 0.
 * sgdnet_cv_covariance_probe: the arguments of sgdnet_cv_*covariance_* (family gaussian: one response; mgaussian:
 * n_classes responses, y n x K column-major), refused in the same words with the same codes.  Fields, Pa = p + K + 1:
 *   mu   one response: p + 2 (as above).  mgaussian: p + 2 K -- the centres, the K sums, the K means
 *   Mg   G x Pa x Pa;  total  Pa x Pa (train_on_rest only)
 *   scale G x p;  mean G x (p + K);  tstat 3 x G;  pen_a, pen_b jobs x n_lambda (alpha | beta, or l2 | l1);  ridge jobs
 *   narrow: Mt  G x (p + 1) x (p + 1) (one response) or G x p x (p + K)
 *   wide:   ld (1);  s, d G x (p + K);  ysd G x K (mgaussian);  S G x p x ld;  Sd G x p;  ct G x p x K
 *   the path kernel's own: W, G jobs x n_lambda x p x K, sweeps, unconverged jobs x n_lambda, tol (1), max_iter (1) */
typedef struct sgdnet_cov_probe sgdnet_cov_probe;
int sgdnet_covariance_path_probe(const double* x_dense, const sgdnet_csc* x_sparse, int64_t n, int64_t p, const double* y, int K,
                                 const double* scale, int centre, int wide, int multi, double mix, int n_lambda,
                                 const double* lambda, int device, double tol, unsigned max_iter, int width,
                                 sgdnet_cov_probe** out);
int sgdnet_covariance_probe(const double* x_dense, const sgdnet_csc* x_sparse, int64_t n, int64_t p, const double* y, int K,
                            const double* scale, int centre, int wide, int multi, double mix, int n_lambda,
                            const double* lambda, int device, sgdnet_cov_probe** out);
int sgdnet_cv_covariance_probe(const double* x_dense, const sgdnet_csc* x_sparse, int64_t n, int64_t p, const double* y,
                               const int32_t* fold, int n_groups, int train_on_rest, const sgdnet_control* ctl, int wide,
                               int n_alpha, const double* alphas, const double* lambdas, sgdnet_cov_probe** out);
/* the number of doubles of field `name` and, through data, where they are; -1: no such field */
int64_t sgdnet_cov_probe_field(const sgdnet_cov_probe* probe, const char* name, const double** data);
void sgdnet_cov_probe_free(sgdnet_cov_probe* probe);

/* ------------------------------------------------------------------------ */
/* Cross-validation in covariance mode (additions only; the ABI version      */
/* stays): every fold fit of every elastic-net mix in ONE call.  Rows carry a */
/* group id fold[i] in [0, n_groups); one pass over x leaves the moments of   */
/* every group on the device, the moments of a training set are pooled from   */
/* them, and all n_alpha * n_groups paths run side by side, one workgroup     */
/* each (sgdnet_amd/csrc/covariance.hip).  Job (alpha a, group g) is by        */
/* definition sgdnet_fit_*(x[T], y[T]) in SGDNET_MODE_COVARIANCE with          */
/* elasticnet_mix = alphas[a] and the user lambdas lambdas[a][.]; T = the rows */
/* of group g (train_on_rest = 0: the reference's convention,                  */
/* R/cv_sgdnet.R:182) or of every other group (train_on_rest = 1).             */
/* control supplies intercept, standardize, max_iter, tol, n_lambda and        */
/* device; family must be gaussian; elasticnet_mix and lambda are ignored in   */
/* favour of the arrays.  No sample is drawn.                                  */
/* SGDNET_EUNSUPPORTED ("mode = covariance needs ..."): more than              */
/* sgdnet_covariance_max_features() features, n_gpus > 1, debug, more than     */
/* 65 535 groups (dense x: row chunks), or group moments -- n_groups x         */
/* (n_features + 2)^2 doubles -- above 64 MiB (which still holds a             */
/* leave-one-out CV of 209 rows at 198 features, of 524 288 rows at 2).        */
/* SGDNET_EINVAL: a fold id outside [0, n_groups), an empty group, a negative  */
/* lambda, a mix outside [0, 1], train_on_rest with one group.                 */
/* ------------------------------------------------------------------------ */
typedef struct sgdnet_cv_cov_result {   /* caller-allocated; job = alpha_index * n_groups + group, L = control.n_lambda */
  double* a0;            /* jobs x L                                                         */
  double* beta;          /* jobs x L x n_features: per job the layout of sgdnet_result.beta  */
  double* dev_ratio;     /* jobs x L                                                         */
  double* return_codes;  /* jobs x L, 0 converged / 1 max_iter sweeps without meeting tol    */
  double* nulldev;       /* jobs: the null deviance of y[T]                                  */
  double* npasses;       /* jobs: coordinate sweeps summed over the path                     */
} sgdnet_cv_cov_result;

/* x n x p column-major, y and fold n; lambdas n_alpha x control.n_lambda, a row per alpha */
int sgdnet_cv_covariance_dense(const double* x, int64_t n, int64_t p, const double* y, const int32_t* fold, int n_groups,
                               int train_on_rest, const sgdnet_control* ctl, int n_alpha, const double* alphas,
                               const double* lambdas, sgdnet_cv_cov_result* out);
int sgdnet_cv_covariance_sparse(const sgdnet_csc* x, const double* y, const int32_t* fold, int n_groups, int train_on_rest,
                                const sgdnet_control* ctl, int n_alpha, const double* alphas, const double* lambdas,
                                sgdnet_cv_cov_result* out);

/* ------------------------------------------------------------------------ */
/* Cross-validation in Newton mode (additions only; the ABI version stays):  */
/* every fold fit of every elastic-net mix in ONE call, all of them advancing */
/* in lock-step.  The arguments are those of sgdnet_cv_covariance_*.  Job     */
/* (alpha a, group g) is by definition sgdnet_fit_*(x[T], y[T]) in            */
/* SGDNET_MODE_NEWTON with elasticnet_mix = alphas[a] and the user lambdas    */
/* lambdas[a][.], T as above: the same preprocessed problem (x_center and     */
/* x_scale over T, the null model of y[T], its null deviance), the same       */
/* stopping rule, constants and accept / halve rule, return_codes and npasses */
/* (state passes of that job) meaning what they mean there.  y holds the      */
/* class codes 0 / 1 of the WHOLE response.  The rows are sorted by group on  */
/* the host and uploaded once; every kernel of the Newton loop runs over all  */
/* jobs at once, each job on the rows of its own training set, and per round  */
/* the host sends one command per job (step / halve / idle, the penalties,    */
/* which iterate is current, where to store an accepted one) and reads all    */
/* records back in one copy (sgdnet_amd/csrc/newton.hip: newton_cv_run).      */
/* control supplies intercept, standardize, max_iter (Newton steps per        */
/* lambda), tol, n_lambda and device; family must be binomial.  No sample is  */
/* drawn.  The same input gives the same bits, and a job's bits do not depend */
/* on which other jobs share the call.                                         */
/* SGDNET_EUNSUPPORTED ("mode = newton needs ..."): a family other than        */
/* binomial, more than sgdnet_newton_max_features() features, n_gpus > 1,      */
/* debug, more than 65 535 jobs, or a workspace -- jobs x (2 n_rows +          */
/* (n_features + 2)^2 + dense x: row chunks x tile pairs x 256) doubles --     */
/* above 1 GiB (which still holds 5 mixes x 10 folds of 1.3 million rows at    */
/* 14 features or of 900 000 rows at 198, and a leave-one-out CV of 300 rows   */
/* at 198 features for 5 mixes).                                               */
/* SGDNET_EINVAL: the cases of sgdnet_cv_covariance_*, a response that is not  */
/* a class code, and a training set that does not hold both classes (the       */
/* message names its group).                                                   */
/* ------------------------------------------------------------------------ */
typedef struct sgdnet_cv_newton_result {   /* caller-allocated; job = alpha_index * n_groups + group, L = control.n_lambda */
  double* a0;            /* jobs x L                                                         */
  double* beta;          /* jobs x L x n_features: per job the layout of sgdnet_result.beta  */
  double* dev_ratio;     /* jobs x L                                                         */
  double* return_codes;  /* jobs x L, 0 converged / 1 max_iter steps without meeting tol     */
  double* nulldev;       /* jobs: the null deviance of y[T]                                  */
  double* npasses;       /* jobs: state passes over the path                                 */
  double* steps;         /* jobs: Newton steps over the path                                 */
  double* halvings;      /* jobs: steps halved (each costs one more state pass)              */
} sgdnet_cv_newton_result;

int sgdnet_cv_newton_dense(const double* x, int64_t n, int64_t p, const double* y, const int32_t* fold, int n_groups,
                           int train_on_rest, const sgdnet_control* ctl, int n_alpha, const double* alphas,
                           const double* lambdas, sgdnet_cv_newton_result* out);
int sgdnet_cv_newton_sparse(const sgdnet_csc* x, const double* y, const int32_t* fold, int n_groups, int train_on_rest,
                            const sgdnet_control* ctl, int n_alpha, const double* alphas, const double* lambdas,
                            sgdnet_cv_newton_result* out);

/* ------------------------------------------------------------------------ */
/* Cross-validation in wide Newton mode (additions only; the ABI version     */
/* stays): sgdnet_cv_newton_* beyond its 198 features.  The arguments and the */
/* result are those of sgdnet_cv_newton_*.  Job (alpha a, group g) is by      */
/* definition sgdnet_fit_*(x[T], y[T]) in SGDNET_MODE_WNEWTON with            */
/* elasticnet_mix = alphas[a] and the user lambdas lambdas[a][.]: the same    */
/* preprocessed problem, stopping rule, constants and accept / halve rule;    */
/* return_codes and npasses mean what they mean there.  What the jobs share:  */
/* x and y, sorted by group and uploaded once, every launch of a round, the   */
/* round's one command upload and one record readback.  What they do not: H   */
/* depends on the iterate, so every job keeps its own moments, its own        */
/* H = M / n_T / (s s') in global memory, diag H and q, and its inner solve   */
/* is one workgroup -- one compute unit -- of its own (sgdnet_amd/csrc/       */
/* newton.hip: wnewton_cv_run).  A job's row chunks are those a single fit    */
/* takes for its rows: the same input gives the same bits, a job's bits do    */
/* not depend on which other jobs share the call, and both widths of the      */
/* inner solve ("wnewton_width") give the same bits.  Sparse x is expanded to */
/* the dense copy a single fit makes: a sparse call gives the bits of the     */
/* dense call on the same matrix.                                             */
/* SGDNET_EUNSUPPORTED ("mode = wnewton needs ..."): a family other than      */
/* binomial, more than sgdnet_wnewton_max_features() features, n_gpus > 1,    */
/* debug, more than 65 535 jobs, a sparse x whose dense copy is above 1 GiB,  */
/* or a workspace -- per job 2 n_rows + (n_features + 2)^2 + row chunks x     */
/* tile pairs x 256 + H + the answers, about 2.5 (n_features + 2)^2 doubles   */
/* -- above 16 GiB (which holds 5 mixes x 10 folds up to 4110 features and    */
/* 25 jobs at the feature limit).  There is no fall-back to                   */
/* sgdnet_cv_newton_* or to separate fits.                                    */
/* SGDNET_EINVAL: the cases of sgdnet_cv_newton_*, and a "wnewton_width"      */
/* that is neither 0, 256 nor 1024.                                           */
/* ------------------------------------------------------------------------ */
typedef sgdnet_cv_newton_result sgdnet_cv_wnewton_result;

int sgdnet_cv_wnewton_dense(const double* x, int64_t n, int64_t p, const double* y, const int32_t* fold, int n_groups,
                            int train_on_rest, const sgdnet_control* ctl, int n_alpha, const double* alphas,
                            const double* lambdas, sgdnet_cv_wnewton_result* out);
int sgdnet_cv_wnewton_sparse(const sgdnet_csc* x, const double* y, const int32_t* fold, int n_groups, int train_on_rest,
                             const sgdnet_control* ctl, int n_alpha, const double* alphas, const double* lambdas,
                             sgdnet_cv_wnewton_result* out);

/* ------------------------------------------------------------------------ */
/* Cross-validation in multi-response covariance mode (additions only; the    */
/* ABI version stays): every fold fit of every elastic-net mix of an          */
/* mgaussian cross-validation in ONE call.  The arguments are those of        */
/* sgdnet_cv_covariance_*, with y n x K column-major and                      */
/* control.n_classes = K.  Job (alpha a, group g) is by definition            */
/* sgdnet_fit_*(x[T], y[T]) in SGDNET_MODE_MCOVARIANCE with                   */
/* elasticnet_mix = alphas[a] and the user lambdas lambdas[a][.], T as above: */
/* the features centred (and scaled) by their moments over T, the responses   */
/* standardised by theirs only with standardize_response (the fit then stays  */
/* on that scale), the null model's intercepts subtracted, the penalties      */
/* (1 - mix) lambda and mix lambda.  One pass over x leaves the               */
/* (n_features + K + 1)^2 moments of every group on the device; the moments   */
/* of a training set are pooled from them and all n_alpha * n_groups block    */
/* coordinate descents run side by side, one workgroup and one compute        */
/* unit's LDS each (sgdnet_amd/csrc/covariance.hip: mcovariance_cv_run).      */
/* control supplies intercept, standardize, standardize_response, max_iter    */
/* (block sweeps per lambda), tol, n_lambda, n_classes and device; family     */
/* must be mgaussian; elasticnet_mix and lambda are ignored in favour of the  */
/* arrays.  No sample is drawn.  The same input gives the same bits, and a    */
/* job's bits do not depend on which other jobs share the call.               */
/* SGDNET_EUNSUPPORTED ("mode = mcovariance needs ..."): a family other than  */
/* mgaussian, n_classes < 2, more than                                        */
/* sgdnet_mcovariance_max_features(n_classes) features, n_gpus > 1, debug,    */
/* more than 65 535 groups (dense x: row chunks), or group moments --         */
/* n_groups x (n_features + n_classes + 1)^2 doubles -- above 64 MiB (which   */
/* still holds a leave-one-out CV of 213 rows at 195 features and 2           */
/* responses, of 327 rows at 63 features and 96 responses).                   */
/* SGDNET_EINVAL: the cases of sgdnet_cv_covariance_*.                        */
/* ------------------------------------------------------------------------ */
typedef struct sgdnet_cv_mcov_result {   /* caller-allocated; job = alpha_index * n_groups + group, L = control.n_lambda, K = control.n_classes */
  double* a0;            /* jobs x L x K                                                     */
  double* beta;          /* jobs x L x K x n_features: per job and lambda the layout of sgdnet_result.beta, entry (k, j) at k + j K */
  double* dev_ratio;     /* jobs x L                                                         */
  double* return_codes;  /* jobs x L, 0 converged / 1 max_iter sweeps without meeting tol    */
  double* nulldev;       /* jobs: the null deviance of y[T]                                  */
  double* npasses;       /* jobs: block sweeps summed over the path                          */
} sgdnet_cv_mcov_result;

/* x n x p column-major, y n x K column-major, fold n; lambdas n_alpha x control.n_lambda, a row per alpha */
int sgdnet_cv_mcovariance_dense(const double* x, int64_t n, int64_t p, const double* y, const int32_t* fold, int n_groups,
                                int train_on_rest, const sgdnet_control* ctl, int n_alpha, const double* alphas,
                                const double* lambdas, sgdnet_cv_mcov_result* out);
int sgdnet_cv_mcovariance_sparse(const sgdnet_csc* x, const double* y, const int32_t* fold, int n_groups, int train_on_rest,
                                 const sgdnet_control* ctl, int n_alpha, const double* alphas, const double* lambdas,
                                 sgdnet_cv_mcov_result* out);

/* ------------------------------------------------------------------------ */
/* Cross-validation in multinomial Newton mode (additions only; the ABI       */
/* version stays): every fold fit of every elastic-net mix in ONE call, all   */
/* of them advancing in lock-step.  The arguments are those of                */
/* sgdnet_cv_newton_*, with control.n_classes = K.  Job (alpha a, group g) is */
/* by definition sgdnet_fit_*(x[T], y[T]) in SGDNET_MODE_MNEWTON with         */
/* n_classes = K, elasticnet_mix = alphas[a] and the user lambdas             */
/* lambdas[a][.], T as above: the same preprocessed problem (x_center and     */
/* x_scale over T; the null model of y[T]: the class-centred logs of T's      */
/* class proportions, or of 1 / K each without an intercept; its null         */
/* deviance), the same stopping rule, constants and accept / halve rule,      */
/* return_codes, npasses (state passes of that job) and the class-centred     */
/* intercepts meaning what they mean there.  y holds the class codes          */
/* 0 .. K - 1 of the WHOLE response.  Sparse x is expanded to the dense copy  */
/* a single fit in this mode makes: a sparse call gives the dense call's      */
/* bits.  The rows are sorted by group on the host and uploaded once; every   */
/* kernel of the loop runs over all jobs at once, each job on the rows of its */
/* own training set with the grids a single fit of that many rows would       */
/* choose, and per round the host sends one command per job (step / halve /   */
/* idle, the penalties, which iterate is current, where to store an accepted  */
/* one) and reads all records back in one copy                                */
/* (sgdnet_amd/csrc/mnewton.hip: mnewton_cv_run).  It is the optimum of the   */
/* separate fit, not its bits: the centres of a training set are formed on    */
/* the host here.  control supplies intercept, standardize, max_iter (Newton  */
/* steps per lambda), tol, n_lambda, n_classes and device; family must be     */
/* multinomial.  No sample is drawn.  The same input gives the same bits, and */
/* a job's bits do not depend on which other jobs share the call.             */
/* SGDNET_EUNSUPPORTED ("mode = mnewton needs ..."): a family other than      */
/* multinomial, n_classes outside 2 .. 99, the grouped penalty, more than     */
/* sgdnet_mnewton_max_features(n_classes) features, n_gpus > 1, debug, a      */
/* dense copy of a sparse x above 1 GiB, more than 65 535 jobs or jobs x      */
/* K (K + 1) / 2 class pairs, or a workspace -- per job rows x K +            */
/* K (K + 1) / 2 x ((n_features + 2)^2 + row chunks x tile pairs x 256) +     */
/* 1024 + (n_lambda + 3) x K (n_features + 1) + 8 doubles, and x and y once   */
/* -- above 1 GiB (which still holds 5 mixes x 10 folds of 30 000 rows each   */
/* at 10 classes and 18 features).                                            */
/* SGDNET_EINVAL: the cases of sgdnet_cv_covariance_*, a response that is not */
/* a class code in 0 .. K - 1, and a training set that holds no row of some   */
/* class (the message names the group and the class).                         */
/* ------------------------------------------------------------------------ */
typedef struct sgdnet_cv_mnewton_result {  /* caller-allocated; job = alpha_index * n_groups + group, L = control.n_lambda, K = control.n_classes */
  double* a0;            /* jobs x L x K: per job the layout of sgdnet_result.a0, the class mean removed */
  double* beta;          /* jobs x L x n_features x K: per job the layout of sgdnet_result.beta, entry (k, j) at k + j K */
  double* dev_ratio;     /* jobs x L                                                         */
  double* return_codes;  /* jobs x L, 0 converged / 1 max_iter steps without meeting tol     */
  double* nulldev;       /* jobs: the null deviance of y[T]                                  */
  double* npasses;       /* jobs: state passes over the path                                 */
  double* steps;         /* jobs: Newton steps over the path                                 */
  double* halvings;      /* jobs: steps halved (each costs one more state pass)              */
} sgdnet_cv_mnewton_result;

int sgdnet_cv_mnewton_dense(const double* x, int64_t n, int64_t p, const double* y, const int32_t* fold, int n_groups,
                            int train_on_rest, const sgdnet_control* ctl, int n_alpha, const double* alphas,
                            const double* lambdas, sgdnet_cv_mnewton_result* out);
int sgdnet_cv_mnewton_sparse(const sgdnet_csc* x, const double* y, const int32_t* fold, int n_groups, int train_on_rest,
                             const sgdnet_control* ctl, int n_alpha, const double* alphas, const double* lambdas,
                             sgdnet_cv_mnewton_result* out);

/* ------------------------------------------------------------------------ */
/* Cross-validation in wide covariance mode (additions only; the ABI version */
/* stays): sgdnet_cv_covariance_* beyond sgdnet_covariance_max_features()     */
/* features.  The arguments and the result are those of                       */
/* sgdnet_cv_covariance_*; job (alpha a, group g) is by definition            */
/* sgdnet_fit_*(x[T], y[T]) in SGDNET_MODE_WCOVARIANCE with elasticnet_mix =   */
/* alphas[a] and the user lambdas lambdas[a][.]: the same optimum, return      */
/* codes and npasses (list sweeps), not the same bits.  One pass over x leaves */
/* the moments of every group, every training set's scaled Gram matrix is     */
/* pooled from them into global memory, and the n_alpha * n_groups paths run   */
/* one workgroup -- one compute unit -- each; jobs beyond the compute units    */
/* queue (sgdnet_amd/csrc/covariance.hip: wcovariance_cv_run).  The option     */
/* wcovariance_width applies as in one fit (another value: SGDNET_EINVAL).     */
/* SGDNET_EUNSUPPORTED ("mode = wcovariance needs ..."): a family other than   */
/* gaussian, more than sgdnet_wcovariance_max_features() features, n_gpus > 1, */
/* debug, more than 65 535 groups (dense x: row chunks), or more than 16 GiB   */
/* of group moments, partial tiles and scaled matrices -- a 10-fold CV at the  */
/* feature limit takes 4.3 GB of it; the message gives the bytes.  There is no */
/* fall-back to sgdnet_cv_covariance_*, to SAGA or to separate fits.           */
/* SGDNET_EINVAL: the cases of sgdnet_cv_covariance_*.                         */
/* ------------------------------------------------------------------------ */
int sgdnet_cv_wcovariance_dense(const double* x, int64_t n, int64_t p, const double* y, const int32_t* fold, int n_groups,
                                int train_on_rest, const sgdnet_control* ctl, int n_alpha, const double* alphas,
                                const double* lambdas, sgdnet_cv_cov_result* out);
int sgdnet_cv_wcovariance_sparse(const sgdnet_csc* x, const double* y, const int32_t* fold, int n_groups, int train_on_rest,
                                 const sgdnet_control* ctl, int n_alpha, const double* alphas, const double* lambdas,
                                 sgdnet_cv_cov_result* out);

/* ------------------------------------------------------------------------ */
/* Cross-validation in wide multi-response covariance mode (additions only;   */
/* the ABI version stays): sgdnet_cv_mcovariance_* beyond                      */
/* sgdnet_mcovariance_max_features(n_classes) features.  The arguments and the */
/* result are those of sgdnet_cv_mcovariance_*; job (alpha a, group g) is by   */
/* definition sgdnet_fit_*(x[T], y[T]) in SGDNET_MODE_WMCOVARIANCE with        */
/* elasticnet_mix = alphas[a] and the user lambdas lambdas[a][.]: the same     */
/* optimum, return codes and npasses (list sweeps), not the same bits.  One    */
/* pass over x leaves the (p + K + 1)^2 moments of every group, every training */
/* set's scaled Gram matrix and c~ are pooled from them into global memory,    */
/* and the n_alpha * n_groups paths run one workgroup -- one compute unit --   */
/* each; jobs beyond the compute units queue (sgdnet_amd/csrc/covariance.hip:  */
/* wmcovariance_cv_run).  The option wmcovariance_width applies as in one fit  */
/* (another value: SGDNET_EINVAL).                                             */
/* SGDNET_EUNSUPPORTED ("mode = wmcovariance needs ..."): a family other than  */
/* mgaussian, n_classes < 2, more than                                         */
/* sgdnet_wmcovariance_max_features(n_classes) features, n_gpus > 1, debug,    */
/* more than 65 535 groups (dense x: row chunks), or more than 16 GiB of group */
/* moments, partial tiles, scaled matrices and c~ -- a 10-fold CV at the limit */
/* of two responses takes 2.9 GB of it; the message gives the bytes.  There is */
/* no fall-back to sgdnet_cv_mcovariance_*, to SAGA or to separate fits.       */
/* SGDNET_EINVAL: the cases of sgdnet_cv_mcovariance_*.                        */
/* ------------------------------------------------------------------------ */
int sgdnet_cv_wmcovariance_dense(const double* x, int64_t n, int64_t p, const double* y, const int32_t* fold, int n_groups,
                                 int train_on_rest, const sgdnet_control* ctl, int n_alpha, const double* alphas,
                                 const double* lambdas, sgdnet_cv_mcov_result* out);
int sgdnet_cv_wmcovariance_sparse(const sgdnet_csc* x, const double* y, const int32_t* fold, int n_groups, int train_on_rest,
                                  const sgdnet_control* ctl, int n_alpha, const double* alphas, const double* lambdas,
                                  sgdnet_cv_mcov_result* out);

#ifdef __cplusplus
}
#endif
#endif /* SGDNET_HIP_H_ */
