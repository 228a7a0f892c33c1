"""Shared by tests/test_kkt_host.py and tests/test_gpu_gradient.py: the numpy definition of the averaged loss
gradient (include/sgdnet_hip.h, sgdnet_gradient_*), seeded problems per family, and the bound on the KKT ratio at
an optimum that test_kkt_host.py records."""
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

# test_kkt_host.py: 10 x the largest figure the oracle's optimum (thresh = 1e-11) leaves over the case matrix, per
# family, capped at 1e-5.  The observed maxima are in that module's docstring.
RATIO_OBSERVED = {"gaussian": 1.5e-9, "binomial": 1.9e-10, "multinomial": 1.9e-10, "mgaussian": 3.7e-10}
INTERCEPT_OBSERVED = {"gaussian": 1.0e-8, "binomial": 4.4e-10, "multinomial": 1.6e-10, "mgaussian": 2.8e-9}
CAP = 1e-5
RATIO_BOUND = {f: min(10.0 * v, CAP) for f, v in RATIO_OBSERVED.items()}
INTERCEPT_BOUND = {f: min(10.0 * v, CAP) for f, v in INTERCEPT_OBSERVED.items()}


def residuals(family, lp, y):
    """r (n, K, L): the family's gradient (reference src/families.h) at the linear predictors lp (n, K, L)."""
    if family == "gaussian":
        return lp - np.asarray(y, dtype=np.float64).reshape(-1, 1, 1)
    if family == "mgaussian":
        return lp - np.asarray(y, dtype=np.float64)[:, :, None]
    if family == "binomial":
        with np.errstate(over="ignore"):
            return 1.0 - np.asarray(y, dtype=np.float64).reshape(-1, 1, 1) - 1.0 / (1.0 + np.exp(lp))
    z = lp - lp.max(axis=1, keepdims=True)
    r = np.exp(z)
    r /= r.sum(axis=1, keepdims=True)
    r[np.arange(lp.shape[0]), np.asarray(y).astype(np.int64), :] -= 1.0
    return r


def numpy_gradient(family, x, y, a0, beta):
    """(G (K, p, L), G0 (K, L), scale (K, L), scale0 (K, L)) from the definition: G[k, j, l] = mean_i x_ij r_ik(l),
    G0 = mean_i r_ik(l); scale[k, l] = max_j mean_i |x_ij| |r_ik(l)| and scale0 = mean_i |r_ik(l)| (the ones column):
    what an entrywise tolerance on G and on G0 multiplies."""
    n, p = x.shape
    K, _, L = beta.shape
    xd = x.toarray() if sp.issparse(x) else np.asarray(x, dtype=np.float64)
    lp = np.einsum("ij,kjl->ikl", xd, beta) + a0[None, :, :]
    r = residuals(family, lp, y)
    G = np.einsum("ij,ikl->kjl", xd, r) / n
    G0 = r.mean(axis=0)
    A = np.einsum("ij,ikl->kjl", np.abs(xd), np.abs(r)) / n
    return G, G0, A.max(axis=1), np.abs(r).mean(axis=0)


def lambda_max(family, x, y, standardize):
    """The lasso's lambda_max (reference src/families.h LambdaMax): below it the path has non-zero coefficients."""
    xd = x.toarray() if sp.issparse(x) else np.asarray(x, dtype=np.float64)
    n = xd.shape[0]
    if standardize:
        sd = xd.std(axis=0)
        xd = (xd - xd.mean(axis=0)) / np.where(sd == 0, 1.0, sd)
    y = np.asarray(y, dtype=np.float64)
    if family == "multinomial":
        Y = (y.reshape(-1, 1) == np.arange(int(y.max()) + 1)).astype(np.float64)
    else:
        Y = y.reshape(n, -1)
    g = xd.T @ (Y - Y.mean(axis=0)) / n
    return float(np.sqrt((g ** 2).sum(axis=1)).max() if family == "mgaussian" else np.abs(g).max())


def as_fit(family, res, alpha):
    """An oracle.fit result as the object sa.kkt_from_gradient reads (family, a0, beta, lambda_, alpha)."""
    return SimpleNamespace(family=family, a0=res["a0"], beta=res["beta"], lambda_=res["lambda"], alpha=alpha)


def problem(family, seed, n=400, p=10, sparse=False):
    """Seeded (x, y): features of different scales and non-zero means (so that standardising matters), a response with
    a non-zero mean (so that the intercept matters)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, p)) * rng.uniform(0.5, 2.0, p) + rng.uniform(-0.5, 0.5, p)
    if sparse:
        x = x * (rng.random((n, p)) < 0.3)
    bt = rng.standard_normal(p) * (rng.random(p) < 0.6)
    if family == "gaussian":
        y = x @ bt + 0.5 * rng.standard_normal(n) + 1.3
    elif family == "binomial":
        y = (rng.random(n) < 1.0 / (1.0 + np.exp(-(0.5 * x @ bt + 0.4)))).astype(np.float64)
    elif family == "multinomial":
        W = rng.standard_normal((p, 3)) * (rng.random((p, 3)) < 0.6)
        s = 0.5 * x @ W + rng.gumbel(size=(n, 3))
        y = s.argmax(axis=1).astype(np.float64)
    else:
        W = rng.standard_normal((p, 2)) * (rng.random((p, 1)) < 0.6)
        y = x @ W + 0.5 * rng.standard_normal((n, 2)) + np.array([0.7, -1.1])
    return (sp.csc_matrix(x) if sparse else x), y
