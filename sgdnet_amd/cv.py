"""cv_sgdnet(): k-fold cross-validation over alpha x lambda; host mirror of the reference's
R/cv_sgdnet.R:113-300.

The n_alpha * nfolds fold fits are independent calls of the same C-ABI entry point
(sgdnet_fit_sparse / sgdnet_fit_dense), so they fan out over the GPUs of a node with no
data-path collective: `devices=[0, 1, ...]` runs them from a thread pool, one fit per device at
a time (ctypes releases the GIL for the duration of the native call).

Two behaviours of the reference are kept because results depend on them, and flagged:
  * R/cv_sgdnet.R:182-183 trains on fold j (`train_ind <- j == foldid`) and scores on the other
    folds; `train_on="rest"` gives the conventional assignment instead.
  * R/cv_sgdnet.R:130 densifies x (`as.matrix`); here x stays sparse unless `densify=True`
    (a 10M x 10k matrix cannot be densified) -- same optimum, different standardisation path.
With one device and an `rng`, fits consume R's generator in the reference's order (full fits,
sample() for the fold ids, fold fits); with several devices every fit gets its own seed.

fold_fits="batched" (mode="covariance" only): the n_alpha * nfolds fold fits are ONE native call
(cv_covariance_fits -> sgdnet_cv_covariance_*): one pass over x leaves the moments of every fold on the
device, every training set's moments are pooled from them and all paths run side by side, one workgroup each.
The full fits, the fold ids, the scoring and the result are those of the default fold_fits="separate".

cv_sgdnet_newton() is the binomial CV whose fits are sgdnet_newton(); its fold_fits="batched" runs all fold fits through
cv_newton_fits -> sgdnet_cv_newton_*: the Newton loops of all jobs advance in lock-step, every kernel launched once per
round over all of them (csrc/newton.hip: newton_cv_run).

cv_sgdnet_wnewton() is the binomial CV whose fits are sgdnet_wnewton() (beyond Newton mode's 198 features); its
fold_fits="batched" runs all fold fits through cv_wnewton_fits -> sgdnet_cv_wnewton_*: the same lock-step loop around the wide
inner solve, every job with its own H in device memory and one workgroup -- one compute unit -- per job and round
(csrc/newton.hip: wnewton_cv_run).

cv_sgdnet_mcovariance() is the mgaussian CV whose fits are sgdnet_mcovariance(); its fold_fits="batched" runs all fold fits
through cv_mcovariance_fits -> sgdnet_cv_mcovariance_*: the group moments of the K responses from one pass, every training
set pooled from them, one workgroup per path (csrc/covariance.hip: mcovariance_cv_run).

cv_sgdnet_mnewton() is the multinomial CV whose fits are sgdnet_mnewton(); its fold_fits="batched" runs all fold fits through
cv_mnewton_fits -> sgdnet_cv_mnewton_*: the multinomial Newton loops of all jobs in lock-step (csrc/mnewton.hip: mnewton_cv_run).

cv_sgdnet_wcovariance() is the gaussian CV whose fits are sgdnet_wcovariance() (beyond covariance mode's 198 features); its
fold_fits="batched" runs all fold fits through cv_wcovariance_fits -> sgdnet_cv_wcovariance_*: the group moments from one pass,
every training set's scaled Gram matrix pooled from them into device memory, one workgroup -- one compute unit -- per path
(csrc/covariance.hip: wcovariance_cv_run).

cv_sgdnet_wmcovariance() is the mgaussian CV whose fits are sgdnet_wmcovariance() (beyond mcovariance mode's feature limit); its
fold_fits="batched" runs all fold fits through cv_wmcovariance_fits -> sgdnet_cv_wmcovariance_*: the group moments of the K
responses from one pass, every training set's scaled Gram matrix and c~ pooled from them into device memory, one workgroup --
one compute unit -- per path (csrc/covariance.hip: wmcovariance_cv_run).
_cv() is the body the seven CVs share; they differ in the fit they inject.
"""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import FAMILIES, MODE_MCOVARIANCE, MODE_MNEWTON, MODE_NEWTON, MODE_WCOVARIANCE, MODE_WMCOVARIANCE, MODE_WNEWTON, MODES, check, dptr
from .api import (SgdnetFit, _levels, sgdnet, sgdnet_mcovariance, sgdnet_mnewton, sgdnet_newton, sgdnet_wcovariance, sgdnet_wmcovariance,
                  sgdnet_wnewton)
from .score import _MEASURES, score
from .solver import RRng


@dataclass
class CvSgdnet:
    alpha: np.ndarray
    lambda_: list
    cv_summary: np.ndarray          # columns: alpha, lambda, mean, sd, ci_lo, ci_up
    cv_raw: list
    name: str
    fit: object
    alpha_min: float
    lambda_min: float
    lambda_1se: float
    foldid: np.ndarray


def r_cut(x, breaks):
    """as.numeric(cut(x, breaks)) for a single number of breaks (R's cut.default)."""
    x = np.asarray(x, dtype=np.float64)
    nb = int(breaks) + 1
    lo, hi = x.min(), x.max()
    dx = hi - lo
    if dx == 0:
        dx = abs(lo)
        b = np.linspace(lo - dx / 1000, hi + dx / 1000, nb)
    else:
        b = np.linspace(lo, hi, nb)
        b[0], b[-1] = lo - dx / 1000, hi + dx / 1000
    return np.searchsorted(b, x, side="left")                    # intervals (b_i, b_i+1], codes 1..breaks


def col_sd(m):
    """R/utils.R:38-46."""
    n = m.shape[0]
    var = np.mean(m ** 2, axis=0) - np.mean(m, axis=0) ** 2
    return np.sqrt(var * n / (n - 1))


def summarize_cv_raw(cv_raw):
    """R/cv_sgdnet.R:286-292: mean, sd, mean - sd, mean + sd per lambda."""
    bar, sd = cv_raw.mean(axis=0), col_sd(cv_raw)
    return np.column_stack([bar, sd, bar - sd, bar + sd])


def find_optimum(summary):
    """R/cv_sgdnet.R:262-276 for one alpha."""
    lam, mean, sd = summary[:, 1], summary[:, 2], summary[:, 3]
    i = int(np.argmin(mean))
    within = mean <= mean[i] + sd[i]
    return dict(alpha_min=summary[i, 0], lambda_min=lam[i], lambda_1se=lam[within].max(), error_min=mean[i])


def cv_covariance_fits(x, y, foldid, alpha, lambda_, train_on="fold", *, maxit=1000, standardize=True, intercept=True,
                       thresh=0.001, device=0):
    """Every fold fit of a gaussian cross-validation in covariance mode from one native call.

    foldid: one label per sample (any values; the folds are np.unique(foldid), in that order).  alpha: one mix or a
    sequence.  lambda_: the penalty strengths, one array per alpha (a single array when alpha is a single number), all
    of one length.  train_on: "fold" (fit on the fold's own rows, the reference's convention) or "rest".
    Returns a list of SgdnetFit, alpha-major: entry a * nfolds + j is sgdnet(x[T], y[T], alpha=alpha[a],
    lambda_=lambda_[a], mode="covariance") for the training set T of fold j."""
    y_enc = np.ascontiguousarray(np.asarray(y), dtype=np.float64).reshape(-1)
    return _native_fold_fits(x, y_enc, foldid, alpha, lambda_, train_on, family="gaussian", classnames=None, maxit=maxit,
                             standardize=standardize, intercept=intercept, thresh=thresh, device=device)


def cv_wcovariance_fits(x, y, foldid, alpha, lambda_, train_on="fold", *, maxit=1000, standardize=True, intercept=True,
                        thresh=0.001, device=0):
    """Every fold fit of a gaussian cross-validation in wide covariance mode from one native call.

    The arguments are cv_covariance_fits's, for up to wcovariance_max_features() features.  Returns a list of SgdnetFit,
    alpha-major: entry a * nfolds + j is sgdnet_wcovariance(x[T], y[T], alpha=alpha[a], lambda_=lambda_[a]) for the
    training set T of fold j (the same optimum, return codes and npasses; not the same bits)."""
    y_enc = np.ascontiguousarray(np.asarray(y), dtype=np.float64).reshape(-1)
    return _native_fold_fits(x, y_enc, foldid, alpha, lambda_, train_on, family="gaussian", classnames=None, maxit=maxit,
                             standardize=standardize, intercept=intercept, thresh=thresh, device=device, wide=True)


def cv_newton_fits(x, y, foldid, alpha, lambda_, train_on="fold", *, maxit=1000, standardize=True, intercept=True,
                   thresh=0.001, device=0):
    """Every fold fit of a binomial cross-validation in Newton mode from one native call, all of them advancing in lock-step.

    The arguments are cv_covariance_fits's; y holds two classes and is encoded once, over all samples, as sgdnet() encodes
    a binomial response (so a fold's class codes are the whole data's).  Returns a list of SgdnetFit, alpha-major: entry
    a * nfolds + j is sgdnet_newton(x[T], y[T], alpha=alpha[a], lambda_=lambda_[a]) for the training set T of fold j;
    its diagnostics hold the job's Newton steps and halvings over the path ("steps", "halvings")."""
    return _binomial_fold_fits(x, y, foldid, alpha, lambda_, train_on, maxit=maxit, standardize=standardize, intercept=intercept,
                               thresh=thresh, device=device, wide=False)


def cv_wnewton_fits(x, y, foldid, alpha, lambda_, train_on="fold", *, maxit=1000, standardize=True, intercept=True,
                    thresh=0.001, device=0):
    """Every fold fit of a binomial cross-validation in wide Newton mode from one native call, all of them advancing in
    lock-step.

    The arguments are cv_newton_fits's, for up to wnewton_max_features() features.  Returns a list of SgdnetFit, alpha-major:
    entry a * nfolds + j is sgdnet_wnewton(x[T], y[T], alpha=alpha[a], lambda_=lambda_[a]) for the training set T of fold j
    (the same optimum, return codes and npasses; not the same bits); its diagnostics hold the job's Newton steps and halvings
    over the path ("steps", "halvings").  Sparse x gives the bits of the dense call on the same matrix."""
    return _binomial_fold_fits(x, y, foldid, alpha, lambda_, train_on, maxit=maxit, standardize=standardize, intercept=intercept,
                               thresh=thresh, device=device, wide=True)


def _binomial_fold_fits(x, y, foldid, alpha, lambda_, train_on, *, maxit, standardize, intercept, thresh, device, wide):
    """cv_newton_fits and cv_wnewton_fits: the response encoded once, over all samples"""
    y_arr = np.asarray(y)
    if y_arr.ndim > 1 and y_arr.shape[1] > 1:
        raise ValueError("response for binomial regression must be one-dimensional.")
    levels, _, codes = _levels(y_arr)
    if levels.size > 2:
        raise ValueError("more than two classes in response. Are you looking for family = 'multinomial'?")
    if levels.size == 1:
        raise ValueError("only one class in response.")
    return _native_fold_fits(x, np.ascontiguousarray(codes), foldid, alpha, lambda_, train_on, family="binomial",
                             classnames=[str(v) for v in levels], maxit=maxit, standardize=standardize, intercept=intercept,
                             thresh=thresh, device=device, wide=wide)


def cv_mcovariance_fits(x, y, foldid, alpha, lambda_, train_on="fold", *, maxit=1000, standardize=True, intercept=True,
                        thresh=0.001, standardize_response=False, device=0):
    """Every fold fit of an mgaussian cross-validation in multi-response covariance mode from one native call.

    The arguments are cv_covariance_fits's; y is n x K with K >= 2 responses.  Returns a list of SgdnetFit, alpha-major:
    entry a * nfolds + j is sgdnet_mcovariance(x[T], y[T], alpha=alpha[a], lambda_=lambda_[a],
    standardize_response=standardize_response) for the training set T of fold j."""
    y_arr = np.asarray(y)
    if y_arr.ndim != 2 or y_arr.shape[1] < 2:
        raise ValueError("response for multivariate Gaussian regression must not be one-dimensional; try family = 'gaussian'.")
    if y_arr.dtype.kind not in "fiub":
        raise ValueError("non-numeric response.")
    return _native_fold_fits(x, np.asfortranarray(y_arr, dtype=np.float64), foldid, alpha, lambda_, train_on, family="mgaussian",
                             classnames=None, maxit=maxit, standardize=standardize, intercept=intercept, thresh=thresh,
                             standardize_response=standardize_response, device=device)


def cv_wmcovariance_fits(x, y, foldid, alpha, lambda_, train_on="fold", *, maxit=1000, standardize=True, intercept=True,
                         thresh=0.001, standardize_response=False, device=0):
    """Every fold fit of an mgaussian cross-validation in wide multi-response covariance mode from one native call.

    The arguments are cv_mcovariance_fits's, for up to wmcovariance_max_features(K) features.  Returns a list of SgdnetFit,
    alpha-major: entry a * nfolds + j is sgdnet_wmcovariance(x[T], y[T], alpha=alpha[a], lambda_=lambda_[a],
    standardize_response=standardize_response) for the training set T of fold j (the same optimum, return codes and
    npasses; not the same bits)."""
    y_arr = np.asarray(y)
    if y_arr.ndim != 2 or y_arr.shape[1] < 2:
        raise ValueError("response for multivariate Gaussian regression must not be one-dimensional; try family = 'gaussian'.")
    if y_arr.dtype.kind not in "fiub":
        raise ValueError("non-numeric response.")
    return _native_fold_fits(x, np.asfortranarray(y_arr, dtype=np.float64), foldid, alpha, lambda_, train_on, family="mgaussian",
                             classnames=None, maxit=maxit, standardize=standardize, intercept=intercept, thresh=thresh,
                             standardize_response=standardize_response, device=device, wide=True)


def cv_mnewton_fits(x, y, foldid, alpha, lambda_, train_on="fold", *, maxit=1000, standardize=True, intercept=True,
                    thresh=0.001, device=0):
    """Every fold fit of a multinomial cross-validation in multinomial Newton mode from one native call, all of them
    advancing in lock-step.

    The arguments are cv_covariance_fits's; y holds K >= 2 classes and is encoded once, over all samples, as sgdnet()
    encodes a multinomial response (so a fold's class codes are the whole data's; a training set without a row of some
    class is refused).  Returns a list of SgdnetFit, alpha-major: entry a * nfolds + j is sgdnet_mnewton(x[T], y[T],
    alpha=alpha[a], lambda_=lambda_[a]) for the training set T of fold j, in the shapes sgdnet_mnewton returns (a0 (K, n_lambda)
    with its class mean removed, beta a list of K (p, n_lambda) arrays); its diagnostics hold the job's Newton steps and
    halvings over the path ("steps", "halvings")."""
    y_arr = np.asarray(y)
    if y_arr.ndim > 1 and y_arr.shape[1] > 1:
        raise ValueError("response for multinomial regression must be one-dimensional.")
    levels, _, codes = _levels(y_arr)
    if levels.size == 1:
        raise ValueError("only one class in response.")
    return _native_fold_fits(x, np.ascontiguousarray(codes), foldid, alpha, lambda_, train_on, family="multinomial",
                             classnames=[str(v) for v in levels], maxit=maxit, standardize=standardize, intercept=intercept,
                             thresh=thresh, device=device, n_classes=int(levels.size))


def _native_fold_fits(x, y_enc, foldid, alpha, lambda_, train_on, *, family, classnames, maxit, standardize, intercept, thresh,
                      device, standardize_response=False, n_classes=1, wide=False):
    """Validation, the native call and the SgdnetFit list behind cv_covariance_fits (gaussian: sgdnet_cv_covariance_*),
    cv_wcovariance_fits (gaussian, wide: sgdnet_cv_wcovariance_*), cv_wmcovariance_fits (mgaussian, wide: sgdnet_cv_wmcovariance_*),
    cv_newton_fits (binomial: sgdnet_cv_newton_*), cv_wnewton_fits (binomial, wide: sgdnet_cv_wnewton_*), cv_mcovariance_fits (mgaussian: sgdnet_cv_mcovariance_*) and cv_mnewton_fits
    (multinomial: sgdnet_cv_mnewton_*, n_classes classes); y_enc: the response as the backend takes it (mgaussian: n x K,
    column-major)."""
    import scipy.sparse as sp

    mnewton = family == "multinomial"
    newton, multi = family == "binomial" or mnewton, family == "mgaussian" or mnewton     # (the Newton loop; K columns of output)
    K = y_enc.shape[1] if family == "mgaussian" else n_classes
    if train_on not in ("fold", "rest"):
        raise ValueError("train_on must be 'fold' or 'rest'")
    if not all(isinstance(v, (bool, np.bool_)) for v in (intercept, standardize)):
        raise ValueError("intercept and standardize must be logical")
    alphas = np.atleast_1d(np.asarray(alpha, dtype=np.float64))
    if np.ndim(alpha) == 0:
        lambda_ = [lambda_]
    rows = [np.asarray(l, dtype=np.float64).reshape(-1) for l in lambda_]
    if len(rows) != alphas.size or rows[0].size == 0 or any(r.size != rows[0].size for r in rows):
        raise ValueError("lambda_ needs one array per alpha, all of one positive length")
    lam = np.ascontiguousarray(rows)
    if np.any(alphas < 0) or np.any(alphas > 1):
        raise ValueError("elastic net mixing parameter (alpha) must be in [0, 1].")
    if np.any(lam < 0):
        raise ValueError("penalty strengths (lambdas) must be positive.")
    if thresh < 0:
        raise ValueError("threshold for stopping criteria cannot be negative.")
    if maxit <= 0:
        raise ValueError("maximum number of iterations cannot be negative or zero.")
    n, p = x.shape
    foldid = np.asarray(foldid).reshape(-1)
    if y_enc.shape[0] != n or foldid.size != n:
        raise ValueError("the number of samples in 'x', 'y' and 'foldid' must match")
    values, fold = np.unique(foldid, return_inverse=True)
    fold = np.ascontiguousarray(fold, dtype=np.int32)
    G, A, nl = values.size, alphas.size, lam.shape[1]

    ctl = _lib.Control()
    ctl.family = FAMILIES[family]
    ctl.intercept, ctl.standardize = int(intercept), int(standardize)
    ctl.standardize_response = int(bool(standardize_response))
    ctl.max_iter, ctl.tol, ctl.n_lambda, ctl.n_classes = int(maxit), float(thresh), nl, K
    ctl.mode = (MODE_MNEWTON if mnewton else (MODE_WNEWTON if wide else MODE_NEWTON) if newton else (MODE_WMCOVARIANCE if wide else MODE_MCOVARIANCE) if multi
                else MODE_WCOVARIANCE if wide else MODES["covariance"])
    ctl.device = int(device)
    jobs = A * G
    a0 = np.zeros((jobs, nl, K) if multi else (jobs, nl))
    beta = np.zeros((jobs, nl, p, K) if multi else (jobs, nl, p))      # (K columns: entry (k, j) at k + j K)
    dev_ratio = np.zeros((jobs, nl))
    rcodes = np.zeros((jobs, nl))
    nulldev = np.zeros(jobs)
    npasses = np.zeros(jobs)
    steps, halvings = np.zeros(jobs), np.zeros(jobs)
    if newton:
        res = (_lib.CvMNewtonResult if mnewton else _lib.CvNewtonResult)(dptr(a0), dptr(beta), dptr(dev_ratio), dptr(rcodes), dptr(nulldev),
                                                                         dptr(npasses), dptr(steps), dptr(halvings))
    else:
        res = (_lib.CvMcovResult if multi else _lib.CvCovResult)(dptr(a0), dptr(beta), dptr(dev_ratio), dptr(rcodes), dptr(nulldev),
                                                                 dptr(npasses))
    tail = (dptr(y_enc), fold.ctypes.data_as(C.POINTER(C.c_int32)), G, int(train_on == "rest"), C.byref(ctl), A, dptr(alphas),
            dptr(lam), C.byref(res))
    L = _lib.load()
    stem = ("sgdnet_cv_mnewton" if mnewton else ("sgdnet_cv_wnewton" if wide else "sgdnet_cv_newton") if newton else ("sgdnet_cv_wmcovariance" if wide else "sgdnet_cv_mcovariance") if multi
            else "sgdnet_cv_wcovariance" if wide else "sgdnet_cv_covariance")
    if sp.issparse(x):
        xs = sp.csc_matrix(x, dtype=np.float64)
        xs.sort_indices()
        colptr = np.ascontiguousarray(xs.indptr, dtype=np.int32)
        rowidx = np.ascontiguousarray(xs.indices, dtype=np.int32)
        vals = np.ascontiguousarray(xs.data, dtype=np.float64)
        csc = _lib.Csc()
        csc.n_rows, csc.n_cols = n, p
        csc.colptr = colptr.ctypes.data_as(C.POINTER(C.c_int32))
        csc.rowidx = rowidx.ctypes.data_as(C.POINTER(C.c_int32))
        csc.values = dptr(vals)
        check(getattr(L, stem + "_sparse")(C.byref(csc), *tail))
    else:
        xd = np.asfortranarray(np.asarray(x, dtype=np.float64).reshape(n, p))
        check(getattr(L, stem + "_dense")(dptr(xd), n, p, *tail))

    counts = np.bincount(fold, minlength=G)
    fits = []
    for a in range(A):
        for j in range(G):
            job = a * G + j
            dfmat = None
            if multi:                                             # the shapes _fit() returns for mgaussian and multinomial
                a0_job = a0[job].T.copy()                         # (K, n_lambda)
                if mnewton:                                       # (as _fit() does: R/sgdnet.R:409-410)
                    a0_job = a0_job - a0_job.mean(axis=0, keepdims=True)
                b = [beta[job, :, :, k].T.copy() for k in range(K)]
                df = (sum(b) != 0).sum(axis=0)
                dfmat = np.vstack([(np.abs(bk) > 0).sum(axis=0) for bk in b])
            else:
                a0_job = a0[job].copy()
                b = beta[job].T.copy()                            # (p, n_lambda)
                df = (b != 0).sum(axis=0)
            fits.append(SgdnetFit(a0=a0_job, beta=b, lambda_=lam[a].copy(), dev_ratio=dev_ratio[job].copy(),
                                  df=df, nulldev=float(nulldev[job]), npasses=float(npasses[job]),
                                  alpha=float(alphas[a]), offset=False, classnames=classnames, grouped=family == "mgaussian",
                                  nobs=int(n - counts[j] if train_on == "rest" else counts[j]), family=family,
                                  dfmat=dfmat, return_codes=rcodes[job].copy(), draws_used=0,
                                  diagnostics=dict(steps=float(steps[job]), halvings=float(halvings[job])) if newton else {}))
    return fits


_BATCHED_FIT_ARGS = ("maxit", "standardize", "intercept", "thresh", "mode", "nlambda", "lambda_min_ratio")


def cv_sgdnet(x, y, alpha=1, lambda_=None, nfolds=10, foldid=None, type_measure="deviance", *, family="gaussian",
              devices=None, rng=None, seed=0, train_on="fold", densify=False, fold_fits="separate", **fit_args):
    import scipy.sparse as sp

    if fold_fits not in ("separate", "batched"):
        raise ValueError("fold_fits must be 'separate' or 'batched'")
    if fold_fits == "batched":
        # one native call covers gaussian fold fits in covariance mode on one device, and nothing else: no silent fallback
        if fit_args.get("mode") != "covariance":
            raise ValueError("fold_fits='batched' needs mode='covariance' (got mode=%r)" % (fit_args.get("mode", "exact"),))
        if family != "gaussian":
            raise ValueError("fold_fits='batched' needs family='gaussian' (got family=%r)" % (family,))
        if devices and len(devices) > 1:
            raise ValueError("fold_fits='batched' needs one device (got devices=%r)" % (list(devices),))
        extra = sorted(set(fit_args) - set(_BATCHED_FIT_ARGS))
        if extra:
            raise ValueError("fold_fits='batched' does not cover the fit argument(s) " + ", ".join(extra))

    def fit_one(xx, yy, lam, a, dev, fit_seed, rng, sequential):
        kw = dict(fit_args)
        if sequential:
            kw["rng"] = rng                       # R's global generator, advanced by every fit
        else:
            kw["seed"] = fit_seed
        return sgdnet(xx, yy, family=family, alpha=float(a), lambda_=lam, device=dev, **kw)

    def batched_fits(xx, yy, foldid, alpha, lam, dev):
        kw = {k: fit_args[k] for k in ("maxit", "standardize", "intercept", "thresh") if k in fit_args}
        return cv_covariance_fits(xx, yy, foldid, alpha, lam, train_on=train_on, device=dev, **kw)

    return _cv(x, y, alpha, lambda_, nfolds, foldid, type_measure, family=family, devices=devices, rng=rng, seed=seed,
               train_on=train_on, densify=densify, fit_one=fit_one, batched_fits=batched_fits if fold_fits == "batched" else None)


def cv_sgdnet_newton(x, y, alpha=1, lambda_=None, nfolds=10, foldid=None, type_measure="deviance", *, rng=None, seed=0,
                     train_on="fold", fold_fits="separate", device=0, nlambda=100, lambda_min_ratio=None, maxit=1000,
                     standardize=True, intercept=True, thresh=0.001):
    """cv_sgdnet(family="binomial") with every fit a sgdnet_newton(): the fold ids, the scoring, the generator and the
    returned CvSgdnet are cv_sgdnet's.  fold_fits="separate" (the default) runs one sgdnet_newton per fold;
    "batched" runs all fold fits of all alphas through ONE native call (cv_newton_fits) with the full fits' lambdas."""
    if fold_fits not in ("separate", "batched"):
        raise ValueError("fold_fits must be 'separate' or 'batched'")
    if train_on not in ("fold", "rest"):
        raise ValueError("train_on must be 'fold' or 'rest'")
    fit_args = dict(maxit=maxit, standardize=standardize, intercept=intercept, thresh=thresh)

    def fit_one(xx, yy, lam, a, dev, fit_seed, rng, sequential):         # (draws nothing: neither the generator nor a seed)
        return sgdnet_newton(xx, yy, alpha=float(a), lambda_=lam, nlambda=nlambda, lambda_min_ratio=lambda_min_ratio, device=dev,
                             **fit_args)

    def batched_fits(xx, yy, foldid, alpha, lam, dev):
        return cv_newton_fits(xx, yy, foldid, alpha, lam, train_on=train_on, device=dev, **fit_args)

    return _cv(x, y, alpha, lambda_, nfolds, foldid, type_measure, family="binomial", devices=[int(device)], rng=rng, seed=seed,
               train_on=train_on, densify=False, fit_one=fit_one, batched_fits=batched_fits if fold_fits == "batched" else None)


def cv_sgdnet_wnewton(x, y, alpha=1, lambda_=None, nfolds=10, foldid=None, type_measure="deviance", *, rng=None, seed=0,
                      train_on="fold", fold_fits="separate", device=0, nlambda=100, lambda_min_ratio=None, maxit=1000,
                      standardize=True, intercept=True, thresh=0.001):
    """cv_sgdnet(family="binomial") with every fit a sgdnet_wnewton(): cv_sgdnet_newton() beyond its feature limit, up to
    wnewton_max_features() features.  fold_fits="separate" (the default) runs one sgdnet_wnewton per fold; "batched" runs all
    fold fits of all alphas through ONE native call (cv_wnewton_fits) with the full fits' lambdas."""
    if fold_fits not in ("separate", "batched"):
        raise ValueError("fold_fits must be 'separate' or 'batched'")
    if train_on not in ("fold", "rest"):
        raise ValueError("train_on must be 'fold' or 'rest'")
    fit_args = dict(maxit=maxit, standardize=standardize, intercept=intercept, thresh=thresh)

    def fit_one(xx, yy, lam, a, dev, fit_seed, rng, sequential):         # (draws nothing: neither the generator nor a seed)
        return sgdnet_wnewton(xx, yy, alpha=float(a), lambda_=lam, nlambda=nlambda, lambda_min_ratio=lambda_min_ratio, device=dev,
                              **fit_args)

    def batched_fits(xx, yy, foldid, alpha, lam, dev):
        return cv_wnewton_fits(xx, yy, foldid, alpha, lam, train_on=train_on, device=dev, **fit_args)

    return _cv(x, y, alpha, lambda_, nfolds, foldid, type_measure, family="binomial", devices=[int(device)], rng=rng, seed=seed,
               train_on=train_on, densify=False, fit_one=fit_one, batched_fits=batched_fits if fold_fits == "batched" else None)


def cv_sgdnet_wcovariance(x, y, alpha=1, lambda_=None, nfolds=10, foldid=None, type_measure="deviance", *, rng=None, seed=0,
                          train_on="fold", fold_fits="separate", device=0, nlambda=100, lambda_min_ratio=None, maxit=1000,
                          standardize=True, intercept=True, thresh=0.001):
    """cv_sgdnet(family="gaussian") with every fit a sgdnet_wcovariance(): the fold ids, the scoring, the generator and the
    returned CvSgdnet are cv_sgdnet's.  fold_fits="separate" (the default) runs one sgdnet_wcovariance per fold;
    "batched" runs all fold fits of all alphas through ONE native call (cv_wcovariance_fits) with the full fits' lambdas."""
    if fold_fits not in ("separate", "batched"):
        raise ValueError("fold_fits must be 'separate' or 'batched'")
    if train_on not in ("fold", "rest"):
        raise ValueError("train_on must be 'fold' or 'rest'")
    fit_args = dict(maxit=maxit, standardize=standardize, intercept=intercept, thresh=thresh)

    def fit_one(xx, yy, lam, a, dev, fit_seed, rng, sequential):         # (draws nothing: neither the generator nor a seed)
        return sgdnet_wcovariance(xx, yy, alpha=float(a), lambda_=lam, nlambda=nlambda, lambda_min_ratio=lambda_min_ratio,
                                  device=dev, **fit_args)

    def batched_fits(xx, yy, foldid, alpha, lam, dev):
        return cv_wcovariance_fits(xx, yy, foldid, alpha, lam, train_on=train_on, device=dev, **fit_args)

    return _cv(x, y, alpha, lambda_, nfolds, foldid, type_measure, family="gaussian", devices=[int(device)], rng=rng, seed=seed,
               train_on=train_on, densify=False, fit_one=fit_one, batched_fits=batched_fits if fold_fits == "batched" else None)


def cv_sgdnet_mcovariance(x, y, alpha=1, lambda_=None, nfolds=10, foldid=None, type_measure="deviance", *, rng=None, seed=0,
                          train_on="fold", fold_fits="separate", device=0, nlambda=100, lambda_min_ratio=None, maxit=1000,
                          standardize=True, intercept=True, thresh=0.001, standardize_response=False):
    """cv_sgdnet(family="mgaussian") with every fit a sgdnet_mcovariance(): the fold ids, the scoring, the generator and the
    returned CvSgdnet are cv_sgdnet's.  For 0 < alpha < 1 this is the cross-validation over an alpha grid that has optima
    to compare (sgdnet_mcovariance()).  fold_fits="separate" (the default) runs one sgdnet_mcovariance per fold; "batched"
    runs all fold fits of all alphas through ONE native call (cv_mcovariance_fits) with the full fits' lambdas."""
    if fold_fits not in ("separate", "batched"):
        raise ValueError("fold_fits must be 'separate' or 'batched'")
    if train_on not in ("fold", "rest"):
        raise ValueError("train_on must be 'fold' or 'rest'")
    fit_args = dict(maxit=maxit, standardize=standardize, intercept=intercept, thresh=thresh, standardize_response=standardize_response)

    def fit_one(xx, yy, lam, a, dev, fit_seed, rng, sequential):         # (draws nothing: neither the generator nor a seed)
        return sgdnet_mcovariance(xx, yy, alpha=float(a), lambda_=lam, nlambda=nlambda, lambda_min_ratio=lambda_min_ratio,
                                  device=dev, **fit_args)

    def batched_fits(xx, yy, foldid, alpha, lam, dev):
        return cv_mcovariance_fits(xx, yy, foldid, alpha, lam, train_on=train_on, device=dev, **fit_args)

    return _cv(x, y, alpha, lambda_, nfolds, foldid, type_measure, family="mgaussian", devices=[int(device)], rng=rng, seed=seed,
               train_on=train_on, densify=False, fit_one=fit_one, batched_fits=batched_fits if fold_fits == "batched" else None)


def cv_sgdnet_wmcovariance(x, y, alpha=1, lambda_=None, nfolds=10, foldid=None, type_measure="deviance", *, rng=None, seed=0,
                           train_on="fold", fold_fits="separate", device=0, nlambda=100, lambda_min_ratio=None, maxit=1000,
                           standardize=True, intercept=True, thresh=0.001, standardize_response=False):
    """cv_sgdnet(family="mgaussian") with every fit a sgdnet_wmcovariance(): cv_sgdnet_mcovariance() beyond its feature
    limit, up to wmcovariance_max_features(K) features.  fold_fits="separate" (the default) runs one sgdnet_wmcovariance per
    fold; "batched" runs all fold fits of all alphas through ONE native call (cv_wmcovariance_fits) with the full fits'
    lambdas."""
    if fold_fits not in ("separate", "batched"):
        raise ValueError("fold_fits must be 'separate' or 'batched'")
    if train_on not in ("fold", "rest"):
        raise ValueError("train_on must be 'fold' or 'rest'")
    fit_args = dict(maxit=maxit, standardize=standardize, intercept=intercept, thresh=thresh, standardize_response=standardize_response)

    def fit_one(xx, yy, lam, a, dev, fit_seed, rng, sequential):         # (draws nothing: neither the generator nor a seed)
        return sgdnet_wmcovariance(xx, yy, alpha=float(a), lambda_=lam, nlambda=nlambda, lambda_min_ratio=lambda_min_ratio,
                                   device=dev, **fit_args)

    def batched_fits(xx, yy, foldid, alpha, lam, dev):
        return cv_wmcovariance_fits(xx, yy, foldid, alpha, lam, train_on=train_on, device=dev, **fit_args)

    return _cv(x, y, alpha, lambda_, nfolds, foldid, type_measure, family="mgaussian", devices=[int(device)], rng=rng, seed=seed,
               train_on=train_on, densify=False, fit_one=fit_one, batched_fits=batched_fits if fold_fits == "batched" else None)


def cv_sgdnet_mnewton(x, y, alpha=1, lambda_=None, nfolds=10, foldid=None, type_measure="deviance", *, rng=None, seed=0,
                      train_on="fold", fold_fits="separate", device=0, nlambda=100, lambda_min_ratio=None, maxit=1000,
                      standardize=True, intercept=True, thresh=0.001):
    """cv_sgdnet(family="multinomial") with every fit a sgdnet_mnewton(): the fold ids, the scoring, the generator and the
    returned CvSgdnet are cv_sgdnet's.  fold_fits="separate" (the default) runs one sgdnet_mnewton per fold;
    "batched" runs all fold fits of all alphas through ONE native call (cv_mnewton_fits) with the full fits' lambdas."""
    if fold_fits not in ("separate", "batched"):
        raise ValueError("fold_fits must be 'separate' or 'batched'")
    if train_on not in ("fold", "rest"):
        raise ValueError("train_on must be 'fold' or 'rest'")
    fit_args = dict(maxit=maxit, standardize=standardize, intercept=intercept, thresh=thresh)

    def fit_one(xx, yy, lam, a, dev, fit_seed, rng, sequential):         # (draws nothing: neither the generator nor a seed)
        return sgdnet_mnewton(xx, yy, alpha=float(a), lambda_=lam, nlambda=nlambda, lambda_min_ratio=lambda_min_ratio, device=dev,
                              **fit_args)

    def batched_fits(xx, yy, foldid, alpha, lam, dev):
        return cv_mnewton_fits(xx, yy, foldid, alpha, lam, train_on=train_on, device=dev, **fit_args)

    return _cv(x, y, alpha, lambda_, nfolds, foldid, type_measure, family="multinomial", devices=[int(device)], rng=rng, seed=seed,
               train_on=train_on, densify=False, fit_one=fit_one, batched_fits=batched_fits if fold_fits == "batched" else None)


def _cv(x, y, alpha, lambda_, nfolds, foldid, type_measure, *, family, devices, rng, seed, train_on, densify, fit_one, batched_fits):
    """The cross-validation behind cv_sgdnet(), cv_sgdnet_newton(), cv_sgdnet_mcovariance(), cv_sgdnet_mnewton(), cv_sgdnet_wnewton(), cv_sgdnet_wcovariance() and cv_sgdnet_wmcovariance(): the full fits, the fold ids, the fold fits, the scores
    and the summary.  fit_one(x, y, lambda, alpha, device, seed, rng, sequential) is a fit; batched_fits(x, y, foldid, alpha,
    lambdas, device), where given, returns every fold fit from one call (alpha-major), else the folds are fitted one by one."""
    import scipy.sparse as sp

    alpha = np.atleast_1d(np.asarray(alpha, dtype=np.float64))
    if not (nfolds > 2 and alpha.size > 0):
        raise ValueError("nfolds > 2, is.numeric(alpha), length(alpha) > 0 are not all TRUE")
    if type_measure not in _MEASURES[family]:
        raise ValueError("'arg' should be one of " + ", ".join(f"'{m}'" for m in _MEASURES[family]))
    if densify and sp.issparse(x):
        x = np.asarray(x.todense())
    if sp.issparse(x):
        x = sp.csr_matrix(x)
    else:
        x = np.asarray(x, dtype=np.float64)
        if x.ndim == 1:
            x = x.reshape(-1, 1)
    y = np.asarray(y)
    n = x.shape[0]
    if nfolds > n:
        raise ValueError("you cannot have more folds than samples.")
    if isinstance(lambda_, list) and lambda_ and isinstance(lambda_[0], (list, tuple, np.ndarray)):
        if len(lambda_) != alpha.size:
            raise ValueError("the length of the lambda list needs to match the number of alpha.")
        lam_in = [np.asarray(l, dtype=np.float64) for l in lambda_]
    elif lambda_ is not None:
        if alpha.size > 1:
            raise ValueError("you need a list of lambdas (or have it set at NULL) when you have multiple alphas.")
        lam_in = [np.asarray(lambda_, dtype=np.float64)]
    else:
        lam_in = [None] * alpha.size

    devices = [0] if not devices else list(devices)
    sequential = len(devices) == 1
    if rng is None:
        rng = RRng(seed)

    def one_fit(xx, yy, lam, a, dev, fit_seed):
        return fit_one(xx, yy, lam, a, dev, fit_seed, rng, sequential)

    fits = [one_fit(x, y, lam_in[i], alpha[i], devices[0], seed + 1 + i) for i in range(alpha.size)]
    lam = [f.lambda_ for f in fits]

    if foldid is None:
        foldid = r_cut(rng.sample(n), nfolds)      # as.numeric(cut(sample(n_samples), nfolds))
    else:
        foldid = np.asarray(foldid)
        if foldid.size != n:
            raise ValueError("the length of `foldid` must match the number of samples")
        nfolds = np.unique(foldid).size
    fold_values = np.arange(1, nfolds + 1) if np.all(np.isin(foldid, np.arange(1, nfolds + 1))) else np.unique(foldid)

    def fold_job(job):
        i, j, worker, fit_seed = job
        dev = devices[worker]
        sel = foldid == fold_values[j]
        train = sel if train_on == "fold" else ~sel
        test = ~train
        fit = one_fit(x[train], y[train], lam[i], alpha[i], dev, fit_seed)
        # R/score.R auc(): stats::runif(2 n) per lambda, in column order, from the global generator -- the draws order
        # equal probabilities AND move the stream the next fold's fit starts from; drawn on the device (sgdnet_auc_*_rng)
        tie_rng = rng if (type_measure == "auc" and sequential) else None
        return i, j, score(fit, x[test], y[test], type_measure, device=dev, rng=tie_rng)

    jobs = [(i, j, (i * nfolds + j) % len(devices), seed + 1000 + i * nfolds + j)
            for i in range(alpha.size) for j in range(nfolds)]               # (alpha, fold, worker, seed)
    cv_raw = [np.full((nfolds, lam[i].size), np.nan) for i in range(alpha.size)]
    if batched_fits is not None:
        # the groups of the native call in the order of fold_values (np.unique sorts, and so does np.arange(1, nfolds + 1))
        fold_fit = batched_fits(x, y, foldid, alpha, lam, devices[0])
        if len(fold_fit) != alpha.size * nfolds:
            raise ValueError("fold_fits='batched' needs every fold to hold a sample")

        def score_job(job):
            i, j = job[0], job[1]
            test = (foldid == fold_values[j]) != (train_on == "fold")
            # (the tie-breaking draws of "auc" are taken fold by fold in the order of the separate fits: see fold_job)
            tie_rng = rng if type_measure == "auc" else None
            return i, j, score(fold_fit[i * nfolds + j], x[test], y[test], type_measure, device=devices[0], rng=tie_rng)
        results = map(score_job, jobs)
    elif sequential:
        results = map(fold_job, jobs)
    else:
        # one worker per entry of `devices` (list a device twice to run two fits on it at a time)
        pools = [ThreadPoolExecutor(max_workers=1) for _ in devices]
        futures = [pools[job[2]].submit(fold_job, job) for job in jobs]
        results = (f.result() for f in futures)
    for i, j, sc in results:
        cv_raw[i][j, :] = sc
    if not sequential:
        for pool in pools:
            pool.shutdown()

    blocks = []
    for i in range(alpha.size):
        blocks.append(np.column_stack([np.full(lam[i].size, alpha[i]), lam[i], summarize_cv_raw(cv_raw[i])]))
    summary = np.vstack(blocks)
    optima = [find_optimum(b) for b in blocks]
    best = int(np.argmin([o["error_min"] for o in optima]))
    if type_measure == "deviance":
        name = {"gaussian": "Mean-Squared Error", "mgaussian": "Mean-Squared Error",
                "binomial": "Binomial Deviance", "multinomial": "Multnomial Deviance"}[family]
    else:
        name = {"mse": "Mean-Squared Error", "mae": "Mean Absolute Error", "class": "Misclassification Error",
                "auc": "AUC"}[type_measure]
    return CvSgdnet(alpha=alpha, lambda_=lam, cv_summary=summary, cv_raw=cv_raw, name=name, fit=fits[best],
                    alpha_min=optima[best]["alpha_min"], lambda_min=optima[best]["lambda_min"],
                    lambda_1se=optima[best]["lambda_1se"], foldid=foldid)
