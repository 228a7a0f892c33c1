"""Optimality (KKT) certificate of a fitted path: how far is every lambda from its optimum?

Two halves, checked separately:

* path_gradient(): the averaged loss gradient at every lambda, on the device (sgdnet_gradient_*,
  csrc/gradient.hip).  It knows nothing of scaling conventions: original x and y, no penalty term.
* kkt_from_gradient(): pure numpy.  Turns that gradient into the residual of the optimality conditions of
  the problem the driver solves, in the units in which the driver penalises:

  The driver (csrc/driver.cpp) fits the preprocessed problem: features (x_j - mean_j) / sd_j when
  standardize (fit_sparse_impl / fit_dense_impl; sparse x is centred implicitly), the gaussian response
  (y - mean(y)) / sd(y) (prepare_response), and the penalty strengths of regularization_path
  (driver.cpp: path.alpha = (1 - mix) lambda / max_scale, path.beta = mix lambda / max_scale, max_scale =
  sd(y) for gaussian and 1 otherwise) with the functor plan_fit picks (fit_plan.hpp: ridge when alpha = 0,
  group lasso for mgaussian, elastic net otherwise).  rescale_into returns b_j = w_j sd(y) / sd_j.
  With g_j the gradient with respect to the standardised coordinate, in the units of y,

      g_j = (G_j - mean_j G0) / sd_j,      c_j = b_j sd_j,

  stationarity of the preprocessed problem, multiplied by sd(y), reads

      g_j + l2 c_j + l1 sign(c_j) = 0  (c_j != 0),    |g_j| <= l1  (c_j = 0),
      l1 = mix lambda,    l2 = (1 - mix) lambda / sd(y)   (sd(y) = 1 unless gaussian),

  the objective tests/test_gpu_parity.py writes out for gaussian fits: RSS / (2n) + lambda ((1 - mix) /
  (2 sd(y)) |b|^2 + mix |b|_1).  Group lasso: the same with row norms over the K responses.

The intercept.  With intercept=True the fitted linear predictor on the original data IS the driver's
(a0 absorbs the centring), and G0 = 0 at the optimum.  With intercept=False the driver holds the intercept
of the PREPROCESSED problem at its null value, and rescale_into returns it as it is: the linear predictor
the driver made stationary is a0 + y_center + sum_j b_j (x_j - mean_j), not a0 + b'x.  evaluation_intercepts()
returns that intercept, the gradient has to be taken there, and kkt() does so.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import FAMILIES, check, dptr
from .api import _levels


def _stacked(fit):
    """(a0 (K, L), beta (K, p, L)) of a fit, Fortran order: the layout of sgdnet_result."""
    beta = fit.beta
    if isinstance(beta, (list, tuple)):
        beta = np.stack([np.asarray(b, dtype=np.float64) for b in beta])
    else:
        beta = np.asarray(beta, dtype=np.float64)
        if beta.ndim == 2:
            beta = beta[None, :, :]
    K, _, L = beta.shape
    a0 = np.asarray(fit.a0, dtype=np.float64).reshape(K, L)
    return np.asfortranarray(a0), np.asfortranarray(beta)


def _encode_response(fit, y):
    """y as sgdnet() hands it to the backend: (n, y_cols), Fortran order; class codes through api._levels."""
    y = np.asarray(y)
    if fit.family in ("binomial", "multinomial"):
        _, _, codes = _levels(y)
        return np.asfortranarray(codes.reshape(-1, 1))
    if fit.family == "mgaussian":
        return np.asfortranarray(y.astype(np.float64).reshape(y.shape[0], -1))
    return np.asfortranarray(y.astype(np.float64).reshape(-1, 1))


def path_gradient(fit, x, y, device=0, a0=None):
    """(G, G0): G[k, j, l] = mean_i x_ij r_ik(l), G0[k, l] = mean_i r_ik(l), r the family's gradient at
    a0[:, l] + beta[:, :, l]' x_i on x and y as they are.  G is (K, p, nlambda), G0 (K, nlambda).
    x: scipy sparse or dense (n, p); y as sgdnet() takes it.  a0: evaluate at these intercepts instead of the
    fit's (evaluation_intercepts)."""
    import scipy.sparse as sp
    a0_fit, beta = _stacked(fit)
    K, p, L = beta.shape
    a0 = a0_fit if a0 is None else np.asfortranarray(np.asarray(a0, dtype=np.float64).reshape(K, L))
    n = x.shape[0]
    if x.shape[1] != p:
        raise ValueError("x has the wrong number of features")
    y_mat = _encode_response(fit, y)
    if y_mat.shape[0] != n:
        raise ValueError("the number of samples in 'x' and 'y' must match")
    G = np.zeros((K, p, L), order="F")
    G0 = np.zeros((K, L), order="F")
    tail = (dptr(y_mat), y_mat.shape[1], FAMILIES[fit.family], K, dptr(a0), dptr(beta), L, int(device), dptr(G), dptr(G0))
    Lh = _lib.load()
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
        check(Lh.sgdnet_gradient_sparse(C.byref(csc), *tail))
    else:
        xd = np.asfortranarray(np.asarray(x, dtype=np.float64).reshape(n, p))
        check(Lh.sgdnet_gradient_dense(dptr(xd), n, p, *tail))
    return G, G0


def feature_moments(x, standardize=True):
    """(mean, sd) of the columns as the fit computes them (population sd, 0 -> 1; driver.cpp fit_sparse_impl /
    col_mean_sd); (0, 1) when the fit does not standardise."""
    import scipy.sparse as sp
    n, p = x.shape
    if not standardize:
        return np.zeros(p), np.ones(p)
    if sp.issparse(x):
        xs = sp.csc_matrix(x, dtype=np.float64)
        mean = np.asarray(xs.sum(axis=0)).ravel() / n
        cnt = np.diff(xs.indptr)
        col = np.repeat(np.arange(p), cnt)
        var = np.bincount(col, weights=(xs.data - mean[col]) ** 2, minlength=p) / n + (n - cnt) * mean ** 2 / n
    else:
        xd = np.asarray(x, dtype=np.float64).reshape(n, p)
        mean = xd.mean(axis=0)
        var = ((xd - mean) ** 2).mean(axis=0)
    sd = np.sqrt(var)
    sd[var == 0] = 1.0
    return mean, sd


def response_moments(fit, y, standardize_response=False):
    """(y_center, y_scale), one entry per response, as prepare_response (driver.cpp) preprocesses y: the gaussian
    response is always centred and scaled; mgaussian only with standardize_response, and then rescale_into leaves
    the coefficients on that scale: y_scale stays 1 and the caller evaluates on the standardised response."""
    a0, _ = _stacked(fit)
    K = a0.shape[0]
    if fit.family == "gaussian":
        yv = np.asarray(y, dtype=np.float64).ravel()
        sd = yv.std()
        return np.array([yv.mean()]), np.array([sd if sd != 0 else 1.0])
    return np.zeros(K), np.ones(K)


def evaluation_intercepts(fit, x_center=None, y_center=None, intercept=True):
    """The intercepts (K, nlambda) at which the driver's problem is stationary (module docstring): the fit's own with
    intercept=True; a0 + y_center - sum_j mean_j b_j otherwise."""
    a0, beta = _stacked(fit)
    if intercept:
        return a0
    K, p, _ = beta.shape
    xc = np.zeros(p) if x_center is None else np.asarray(x_center, dtype=np.float64)
    yc = np.zeros(K) if y_center is None else np.asarray(y_center, dtype=np.float64).reshape(K)
    return np.asfortranarray(a0 + yc[:, None] - np.einsum("j,kjl->kl", xc, beta))


def kkt_from_gradient(G, G0, fit, x_center=None, x_scale=None, y_scale=None, standardize=True, intercept=True):
    """Optimality residual per lambda from the averaged loss gradient (pure numpy, no device).

    G (K, p, nlambda), G0 (K, nlambda): path_gradient's, taken at evaluation_intercepts().  x_center / x_scale: the
    feature means and sds of the fit (feature_moments; needed when standardize), y_scale: sd(y) of a gaussian fit
    (response_moments; 1 otherwise).  Returns {"coef", "intercept", "ratio"}, arrays of nlambda entries:
    coef = the largest violation over the coefficients (units of y per unit of standardised feature), intercept =
    max_k |G0[k]| (multinomial: after removing the class mean, the intercepts being defined up to a constant; 0
    with intercept=False), ratio = coef / lambda."""
    _, beta = _stacked(fit)
    K, p, L = beta.shape
    G = np.asarray(G, dtype=np.float64).reshape(K, p, L)
    G0 = np.asarray(G0, dtype=np.float64).reshape(K, L)
    lam = np.asarray(fit.lambda_, dtype=np.float64).reshape(L)
    mix = float(fit.alpha)
    if standardize:
        if x_center is None or x_scale is None:
            raise ValueError("standardize=True needs the feature means and sds of the fit (feature_moments)")
        m = np.asarray(x_center, dtype=np.float64).reshape(1, p, 1)
        s = np.asarray(x_scale, dtype=np.float64).reshape(1, p, 1)
        g = (G - m * G0[:, None, :]) / s
        c = beta * s
    else:
        g, c = G, beta
    ys = 1.0 if y_scale is None else float(np.max(np.asarray(y_scale, dtype=np.float64)))     # driver.cpp: max_scale
    l1 = (mix * lam).reshape(1, 1, L)
    l2 = ((1.0 - mix) * lam / ys).reshape(1, 1, L)
    if mix == 0.0:                                              # fit_plan.hpp plan_fit: the ridge functor
        viol = np.abs(g + l2 * c)
    elif fit.family == "mgaussian":                             # group lasso: rows over the K responses
        nrm = np.sqrt((c ** 2).sum(axis=0, keepdims=True))
        live = nrm > 0
        unit = np.divide(c, nrm, out=np.zeros_like(c), where=live)
        on = np.sqrt(((g + l2 * c + l1 * unit) ** 2).sum(axis=0, keepdims=True))
        off = np.maximum(np.sqrt((g ** 2).sum(axis=0, keepdims=True)) - l1, 0.0)
        viol = np.where(live, on, off)
    else:
        viol = np.where(c != 0, np.abs(g + l2 * c + l1 * np.sign(c)), np.maximum(np.abs(g) - l1, 0.0))
    coef = viol.reshape(-1, L).max(axis=0)
    if not intercept:
        icpt = np.zeros(L)
    elif fit.family == "multinomial":
        icpt = np.abs(G0 - G0.mean(axis=0, keepdims=True)).max(axis=0)
    else:
        icpt = np.abs(G0).max(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(lam > 0, coef / lam, np.where(coef > 0, np.inf, 0.0))
    return {"coef": coef, "intercept": icpt, "ratio": ratio}


def kkt(fit, x, y, standardize=True, intercept=True, standardize_response=False, device=0):
    """The optimality certificate of a fitted path: kkt_from_gradient on the device's path_gradient.  standardize,
    intercept and standardize_response are the fit's (SgdnetFit does not record them; sgdnet()'s defaults)."""
    x_center, x_scale = feature_moments(x, standardize)
    y_center, y_scale = response_moments(fit, y, standardize_response)
    if fit.family == "mgaussian" and standardize_response:      # the coefficients live on the standardised response
        yv = np.asarray(y, dtype=np.float64)
        sd = yv.std(axis=0)
        y = (yv - yv.mean(axis=0)) / np.where(sd == 0, 1.0, sd)
    a0 = evaluation_intercepts(fit, x_center, y_center, intercept)
    G, G0 = path_gradient(fit, x, y, device=device, a0=a0)
    return kkt_from_gradient(G, G0, fit, x_center=x_center, x_scale=x_scale, y_scale=y_scale, standardize=standardize,
                             intercept=intercept)
