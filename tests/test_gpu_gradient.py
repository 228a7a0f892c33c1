"""sgdnet_gradient_sparse / _dense (csrc/gradient.hip) through sa.path_gradient, and sa.kkt end to end.

Parity with the numpy definition (tests/kkt_reference.py), entrywise, with the tolerance
    1e-11 * max_j (1/n) sum_i |x_ij| |r_ik|        (G0: 1e-11 * (1/n) sum_i |r_ik|)
computed here: f64 summation error is at most n 2^-53 of the absolute sum (3e-14 at n = 257), the device's and
numpy's exp / log differ by a few ulp of the residual; the tolerance leaves a margin of 30 x and more.
Shapes: one sample past a 256-thread block, one column past 64 and 128 lanes, every short column length around the
16- and 64-lane groups, both group widths (nnz <= 32 p takes the 16-lane groups), more pairs than one chunk holds."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp

import kkt_reference as KR

pytestmark = pytest.mark.gpu
RTOL = 1e-11


@pytest.fixture(scope="module")
def sa():
    import torch  # noqa: F401  -- before libsgdnet_hip.so (sgdnet_amd/_lib.py)
    import sgdnet_amd
    if sgdnet_amd.load().sgdnet_device_count() < 1:
        pytest.fail("GPU tests need a HIP device; the backend has no CPU fallback")
    return sgdnet_amd


def _response(rng, family, n, K):
    if family == "gaussian":
        return rng.standard_normal(n) + 0.5
    if family == "binomial":
        y = (rng.random(n) < 0.5).astype(np.float64)
        y[:2] = (0.0, 1.0)
        return y
    if family == "multinomial":
        y = rng.integers(0, K, n).astype(np.float64)
        y[:K] = np.arange(K)                       # every class present: the codes are the levels
        return y
    return rng.standard_normal((n, K)) + np.arange(K)


def _coefficients(rng, K, p, L, size=0.5):
    """Not an optimum: random coefficients with exact zeros, L lambda columns."""
    beta = size * rng.standard_normal((K, p, L)) * (rng.random((K, p, L)) < 0.6)
    return np.asfortranarray(rng.standard_normal((K, L))), np.asfortranarray(beta)


def _fit(family, a0, beta):
    return SimpleNamespace(family=family, a0=a0, beta=beta, lambda_=np.ones(beta.shape[2]), alpha=0.5)


def _check(sa, family, x, y, a0, beta):
    G, G0 = sa.path_gradient(_fit(family, a0, beta), x, y)
    Gn, G0n, scale, scale0 = KR.numpy_gradient(family, x, y, a0, beta)
    assert G.shape == beta.shape and G0.shape == a0.shape
    err = np.abs(G - Gn) / np.maximum(scale[:, None, :], 1e-300)
    err0 = np.abs(G0 - G0n) / np.maximum(scale0, 1e-300)
    print(f"gradient {family} {x.shape} K={beta.shape[0]} L={beta.shape[2]}: err / scale {err.max():.2e} (G) {err0.max():.2e} (G0)")
    assert (np.abs(G - Gn) <= RTOL * scale[:, None, :]).all()
    assert (np.abs(G0 - G0n) <= RTOL * scale0).all()
    return G, G0


FAMILY_K = [("gaussian", 1), ("binomial", 1), ("multinomial", 3), ("mgaussian", 2), ("mgaussian", 17)]


@pytest.mark.parametrize("family,K", FAMILY_K)
@pytest.mark.parametrize("p,density", [(65, 0.3), (130, 0.05)])
def test_sparse_matches_numpy(sa, family, K, p, density):
    rng = np.random.default_rng(100 + p + K)
    n = 257
    x = sp.random(n, p, density=density, random_state=7 + p, data_rvs=rng.standard_normal).tocsc()
    assert (x.nnz <= 32 * p) == (density < 0.1)          # both group widths of the column reduction
    a0, beta = _coefficients(rng, K, p, 5)
    _check(sa, family, x, _response(rng, family, n, K), a0, beta)


def _column_lengths_matrix(rng, n, lengths):
    cols = []
    for m in lengths:
        col = np.zeros(n)
        rows = rng.choice(np.arange(1, n), size=m, replace=False) if m < n else np.arange(n)      # row 0 stays empty
        col[rows] = rng.standard_normal(m) + 0.2
        cols.append(col)
    return sp.csc_matrix(np.stack(cols, axis=1))


@pytest.mark.parametrize("family,K", [("gaussian", 1), ("multinomial", 3)])
@pytest.mark.parametrize("full_column", [False, True])
def test_sparse_column_lengths_around_the_group_widths(sa, family, K, full_column):
    rng = np.random.default_rng(5)
    n = 257
    lengths = [0, 1, 15, 16, 17, 63, 64, 65] + ([n] if full_column else [])
    x = _column_lengths_matrix(rng, n, lengths)
    assert list(np.diff(x.indptr)) == lengths
    if not full_column:
        assert x[0].nnz == 0                             # an empty row next to the empty column
    a0, beta = _coefficients(rng, K, len(lengths), 5)
    G, _ = _check(sa, family, x, _response(rng, family, n, K), a0, beta)
    assert (G[:, 0, :] == 0).all()                       # the empty column


def test_binomial_extreme_linear_predictors(sa):
    rng = np.random.default_rng(6)
    n, p = 257, 65
    x = sp.random(n, p, density=0.3, random_state=3, data_rvs=rng.standard_normal).tocsc()
    a0, beta = _coefficients(rng, 1, p, 5)
    a0[0, :] = (-40.0, 40.0, 0.0, -700.0, 700.0)         # exp() saturates on both sides
    y = _response(rng, "binomial", n, 1)
    G, G0 = _check(sa, "binomial", x, y, a0, beta)
    assert np.isfinite(G).all() and np.isfinite(G0).all()


def test_one_sample_one_feature(sa):
    x = sp.csc_matrix(np.array([[1.5]]))
    a0, beta = np.asfortranarray([[0.25, -1.0]]), np.asfortranarray(np.array([[[2.0, 0.0]]]))
    G, G0 = _check(sa, "gaussian", x, np.array([0.75]), a0, beta)
    assert np.allclose(G0[0], [0.25 + 3.0 - 0.75, -1.0 - 0.75], rtol=1e-15)
    _check(sa, "gaussian", x.toarray(), np.array([0.75]), a0, beta)


@pytest.mark.parametrize("family,K", FAMILY_K)
@pytest.mark.parametrize("n,p", [(257, 65), (33, 3)])
def test_dense_matches_numpy(sa, family, K, n, p):
    rng = np.random.default_rng(200 + n + K)
    x = rng.standard_normal((n, p)) * (rng.random((n, p)) < 0.8)
    a0, beta = _coefficients(rng, K, p, 5, size=0.2)
    _check(sa, family, x, _response(rng, family, n, K), a0, beta)


def test_more_pairs_than_one_chunk(sa):
    """1050 (lambda, class) pairs: every lambda column equals the one computed alone, bit for bit (the arithmetic of a
    column does not depend on its chunk)."""
    rng = np.random.default_rng(8)
    n, p, K, L = 64, 7, 3, 350
    x = sp.random(n, p, density=0.5, random_state=4, data_rvs=rng.standard_normal).tocsc()
    y = _response(rng, "multinomial", n, K)
    a0, beta = _coefficients(rng, K, p, L)
    G, G0 = _check(sa, "multinomial", x, y, a0, beta)
    for l in range(L):
        Gl, G0l = sa.path_gradient(_fit("multinomial", a0[:, l:l + 1], beta[:, :, l:l + 1]), x, y)
        assert np.array_equal(Gl[:, :, 0], G[:, :, l]) and np.array_equal(G0l[:, 0], G0[:, l]), l


@pytest.mark.parametrize("sparse", [True, False])
def test_two_calls_return_the_same_bits(sa, sparse):
    rng = np.random.default_rng(9)
    n, p, K = 1031, 130, 3
    x = sp.random(n, p, density=0.2, random_state=5, data_rvs=rng.standard_normal).tocsc()
    x = x if sparse else x.toarray()
    y = _response(rng, "multinomial", n, K)
    a0, beta = _coefficients(rng, K, p, 5)
    first = sa.path_gradient(_fit("multinomial", a0, beta), x, y)
    again = sa.path_gradient(_fit("multinomial", a0, beta), x, y)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])


def test_errors(sa):
    from sgdnet_amd import _lib
    from sgdnet_amd._lib import dptr
    L = sa.load()
    n, p, K = 6, 2, 3
    x = np.asfortranarray(np.arange(12, dtype=np.float64).reshape(n, p))
    a0, beta = np.zeros((K, 1), order="F"), np.zeros((K, p, 1), order="F")
    G, G0 = np.zeros((K, p, 1), order="F"), np.zeros((K, 1), order="F")
    y = np.array([0.0, 1.0, 2.0, 0.0, 1.0, 2.0])
    call = lambda yy, g: L.sgdnet_gradient_dense(dptr(x), n, p, dptr(yy), 1, _lib.FAMILIES["multinomial"], K, dptr(a0),  # noqa: E731
                                                 dptr(beta), 1, 0, g, dptr(G0))
    assert call(y, dptr(G)) == 0
    y_bad = y.copy()
    y_bad[3] = float(K)                                  # a class code equal to K
    assert call(y_bad, dptr(G)) == -1
    assert b"class code" in L.sgdnet_last_error()
    assert call(y, None) == -1                           # a null G
    xs = sp.csc_matrix(x)
    csc = _lib.Csc()
    csc.n_rows, csc.n_cols = n, p
    colptr, rowidx = xs.indptr.astype(np.int32), xs.indices.astype(np.int32)
    csc.colptr, csc.rowidx = colptr.ctypes.data_as(C.POINTER(C.c_int32)), rowidx.ctypes.data_as(C.POINTER(C.c_int32))
    csc.values = dptr(xs.data)
    tail = (1, _lib.FAMILIES["multinomial"], K, dptr(a0), dptr(beta), 1, 0)
    assert L.sgdnet_gradient_sparse(C.byref(csc), dptr(y), *tail, dptr(G), dptr(G0)) == 0
    assert L.sgdnet_gradient_sparse(C.byref(csc), dptr(y_bad), *tail, dptr(G), dptr(G0)) == -1
    assert L.sgdnet_gradient_sparse(C.byref(csc), dptr(y), *tail, None, dptr(G0)) == -1
    assert L.sgdnet_gradient_sparse(None, dptr(y), *tail, dptr(G), dptr(G0)) == -1


# ---- end to end: fit, then certify ------------------------------------------------------------------------------
END_TO_END = {
    "binomial": dict(sparse=True, standardize=False, alpha=0.5),
    "gaussian": dict(sparse=False, standardize=True, alpha=0.5),
    "multinomial": dict(sparse=False, standardize=False, alpha=0.5),
}


@pytest.mark.parametrize("mode,batch", [("exact", 0), ("batched", 64)])
@pytest.mark.parametrize("family", list(END_TO_END))
def test_certificate_of_a_fit(sa, family, mode, batch):
    c = END_TO_END[family]
    x, y = KR.problem(family, 21, n=300, p=8, sparse=c["sparse"])
    lam = KR.lambda_max(family, x, y, c["standardize"]) * np.array([0.5, 0.15, 0.04]) / c["alpha"]
    kw = dict(family=family, alpha=c["alpha"], lambda_=lam, standardize=c["standardize"], maxit=5000, seed=2, mode=mode,
              batch=batch)
    fit = sa.sgdnet(x, y, thresh=1e-10, **kw)
    assert (fit.return_codes == 0).all()
    out = sa.kkt(fit, x, y, standardize=c["standardize"])
    print(f"kkt of a {mode} fit, {family}: ratio {out['ratio']} intercept {out['intercept']}")
    # the same certificate from numpy's gradient
    x_center, x_scale = sa.feature_moments(x, c["standardize"])
    _, y_scale = sa.response_moments(fit, y)
    a0 = sa.evaluation_intercepts(fit)
    beta = np.stack(fit.beta) if isinstance(fit.beta, list) else fit.beta[None]
    Gn, G0n, scale, scale0 = KR.numpy_gradient(family, x, y, np.asarray(a0).reshape(beta.shape[0], -1), beta)
    ref = sa.kkt_from_gradient(Gn, G0n, fit, x_center=x_center, x_scale=x_scale, y_scale=y_scale, standardize=c["standardize"])
    # an entry of the standardised gradient is (G_j - mean_j G0) / sd_j: the parity tolerance carried through it
    tol = RTOL * ((scale + np.abs(x_center).max() * scale0) / x_scale.min()).max(axis=0)
    assert (np.abs(out["coef"] - ref["coef"]) <= tol).all()
    assert (np.abs(out["intercept"] - ref["intercept"]) <= 2 * RTOL * scale0.max(axis=0)).all()
    assert out["ratio"].max() < KR.RATIO_BOUND[family]
    # a loose fit of the same problem is told apart
    loose = sa.sgdnet(x, y, thresh=1e-2, **kw)
    out_loose = sa.kkt(loose, x, y, standardize=c["standardize"])
    print(f"   thresh 1e-2: ratio {out_loose['ratio']}")
    assert out_loose["ratio"][-1] > out["ratio"][-1]
