"""mode="covariance" (SGDNET_MODE_COVARIANCE, sgdnet_amd/csrc/covariance.hip): the gaussian path of one response solved
to its optimum from the device's centred X'X and X'y.  Checked against the optimality conditions of the problem the
driver solves (sa.kkt: device gradient on the data as it came + the numpy conventions of sgdnet_amd/kkt.py), not
against another solver's iterates; the shapes sit at the kernels' edges (tile, wavefront, one workgroup's LDS).

numpy_cd_path() below restates the algorithm in numpy; tests/test_covariance_host.py checks on the CPU that this
restatement reproduces scikit-learn and that its optimum stays inside the bound used here for the same inputs."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# The project's optimality bound, restated from tests/test_gpu_parity.py (test_config4_ridge_and_lasso_kkt_at_size:
# "np.abs(g + lam * a * sign(w)).max() < 1e-8 * lam"): KKT residual <= 1e-8 * lambda.
KKT_BOUND = 1e-8
# Coefficient tolerance against the CPU oracle (SAGA at thresh = 1e-9) on the abalone path of
# test_same_optimum_as_the_oracle_on_abalone, relative to max|beta|: 10 x the oracle's own change between thresh = 1e-9
# and thresh = 1e-11, measured 8.26e-9 (its distance from the optimum at that thresh; the measurement is
# test_covariance_host.py::test_oracle_distance_from_its_optimum_on_abalone).
ORACLE_REL_CHANGE = 8.3e-9
ORACLE_TOL = 10 * ORACLE_REL_CHANGE
ABALONE = dict(alpha=0.5, nlambda=12, lambda_min_ratio=1e-2)
ORACLE_THRESH = 1e-9

SHAPES = [(2, 1), (37, 2), (63, 15), (65, 17), (1003, 33), (300, None)]     # None: sgdnet_covariance_max_features()
NONMONOTONE = [0.3, 0.02, 0.8, 0.1, 0.05]


def pmax():
    import sgdnet_amd as sa
    return sa.covariance_max_features()


def problem(n, p, sparse, seed=0):
    """x with columns of different means and scales (sparse: ~35 % stored, the first row always), y = x B + noise."""
    rng = np.random.default_rng(1000 * seed + 7 * n + p)
    x = rng.standard_normal((n, p)) * rng.uniform(0.5, 3.0, p) + rng.uniform(-2.0, 2.0, p)
    if sparse:
        keep = rng.random((n, p)) < 0.35
        keep[0, :] = True
        x = x * keep
    B = rng.standard_normal(p) * (rng.random(p) < 0.5)
    y = x @ B + 0.5 * rng.standard_normal(n) + 1.5
    return (sp.csc_matrix(x) if sparse else x), y


def numpy_cd_path(x, y, lam, mix, standardize=True, intercept=True, tol=1e-13, max_sweeps=200000):
    """Cyclic coordinate descent with covariance updates in the driver's units (sgdnet_amd/kkt.py): (a0, beta (p, L))."""
    x = np.asarray(x.todense()) if sp.issparse(x) else np.asarray(x, dtype=float)
    n, p = x.shape
    ym, ys = y.mean(), (y.std() if y.std() != 0 else 1.0)
    mean = x.mean(axis=0)
    var = ((x - mean) ** 2).mean(axis=0)
    sd = np.where(var == 0, 1.0, np.sqrt(var)) if standardize else np.ones(p)
    mu = mean if (standardize or intercept) else np.zeros(p)
    xt, yt = (x - mu) / sd, (y - ym) / ys
    S, c = xt.T @ xt / n, xt.T @ yt / n
    w, a0, beta = np.zeros(p), [], []
    for l in lam:
        l1, l2 = mix * l / ys, (1 - mix) * l / ys
        g = S @ w - c
        for _ in range(max_sweeps):
            change = 0.0
            for j in range(p):
                z, den = S[j, j] * w[j] - g[j], S[j, j] + l2
                nw = (z if mix == 0 else np.sign(z) * max(abs(z) - l1, 0.0)) / den if den > 0 else 0.0
                d = nw - w[j]
                if d != 0.0:
                    w[j] = nw
                    g += S[:, j] * d
                    change = max(change, abs(d))
            if change <= tol * np.abs(w).max():
                break
        beta.append(w * ys / sd)
        a0.append(ym - mean @ beta[-1] if intercept else 0.0)
    return np.array(a0), np.array(beta).T


def numpy_kkt(a0, beta, x, y, lam, mix, standardize, intercept):
    """sa.kkt without the device: the gradient of the gaussian loss in numpy, then kkt_from_gradient."""
    import sgdnet_amd as sa
    fit = SimpleNamespace(a0=np.asarray(a0), beta=np.asarray(beta), lambda_=np.asarray(lam, dtype=float), alpha=mix, family="gaussian")
    xc, xs = sa.feature_moments(x, standardize)
    yc, ysc = sa.response_moments(fit, y)
    xd = np.asarray(x.todense()) if sp.issparse(x) else np.asarray(x, dtype=float)
    ev = sa.evaluation_intercepts(fit, xc, yc, intercept)                       # (1, L)
    r = ev + xd @ fit.beta - np.asarray(y, dtype=float)[:, None]                # (n, L)
    G, G0 = (xd.T @ r / len(y))[None], r.mean(axis=0)[None]
    return sa.kkt_from_gradient(G, G0, fit, x_center=xc, x_scale=xs, y_scale=ysc, standardize=standardize, intercept=intercept)


def assert_optimal(k, lam, what):
    print(what, "ratio max %.3g intercept/lambda max %.3g" % (np.max(k["ratio"]), np.max(k["intercept"] / np.maximum(lam, 1e-300))))
    assert (k["ratio"] <= KKT_BOUND).all(), (what, k["ratio"])
    assert (k["intercept"] <= KKT_BOUND * lam).all(), (what, k["intercept"], lam)


@pytest.fixture(scope="module")
def sa():
    import torch  # noqa: F401
    import sgdnet_amd
    if sgdnet_amd.load().sgdnet_device_count() < 1:
        pytest.fail("GPU tests need a HIP device; the backend has no CPU fallback")
    return sgdnet_amd


# ---- (i) optimality across the envelope ----

@pytest.mark.parametrize("mix", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_automatic_path_is_optimal(sa, shape, sparse, mix):
    n, p = shape[0], shape[1] or pmax()
    x, y = problem(n, p, sparse)
    for intercept in (True, False):
        for standardize in (True, False):
            fit = sa.sgdnet(x, y, alpha=mix, nlambda=20, lambda_min_ratio=1e-2, thresh=1e-12, maxit=1_000_000,
                            intercept=intercept, standardize=standardize, mode="covariance")
            assert (fit.return_codes == 0).all() and fit.draws_used == 0 and np.isfinite(fit.dev_ratio).all()
            k = sa.kkt(fit, x, y, standardize=standardize, intercept=intercept)
            assert_optimal(k, fit.lambda_, (n, p, sparse, mix, intercept, standardize))     # no lambda dropped


@pytest.mark.parametrize("sparse", [False, True])
def test_user_lambdas_need_not_be_monotone(sa, sparse):
    x, y = problem(65, 17, sparse, seed=1)
    fit = sa.sgdnet(x, y, alpha=0.5, lambda_=NONMONOTONE, thresh=1e-12, maxit=1_000_000, mode="covariance")
    assert np.array_equal(fit.lambda_, NONMONOTONE) and (fit.return_codes == 0).all()
    assert_optimal(sa.kkt(fit, x, y), fit.lambda_, ("user lambdas", sparse))
    # every lambda's optimum is its own: the same values in decreasing order give the same coefficients
    order = np.argsort(NONMONOTONE)[::-1]
    mono = sa.sgdnet(x, y, alpha=0.5, lambda_=np.array(NONMONOTONE)[order], thresh=1e-12, maxit=1_000_000, mode="covariance")
    assert np.abs(fit.beta[:, order] - mono.beta).max() <= 1e-9 * np.abs(mono.beta).max()


def test_max_iter_is_reported(sa):
    x, y = problem(65, 17, False, seed=2)
    fit = sa.sgdnet(x, y, alpha=0.5, nlambda=5, lambda_min_ratio=1e-2, thresh=1e-14, maxit=2, mode="covariance")
    assert (fit.return_codes[1:] == 1).all() and 2 * 4 + 1 <= fit.npasses <= 2 * 5


# ---- (ii) the same optimum as the existing solver ----

def test_same_lambdas_as_exact_mode_on_abalone(sa):
    ab = np.load(os.path.join(GOLD, "abalone.npz"))
    cov = sa.sgdnet(ab["x"], ab["y"], mode="covariance", **ABALONE)
    exact = sa.sgdnet(ab["x"], ab["y"], mode="exact", **ABALONE)
    assert cov.lambda_.tobytes() == exact.lambda_.tobytes()
    assert cov.nulldev == exact.nulldev


def test_same_optimum_as_the_oracle_on_abalone(sa, oracle):
    ab = np.load(os.path.join(GOLD, "abalone.npz"))
    ref = oracle.fit(ab["x"], ab["y"], family="gaussian", thresh=ORACLE_THRESH, maxit=100000, seed=1, **ABALONE)
    fit = sa.sgdnet(ab["x"], ab["y"], mode="covariance", thresh=1e-12, maxit=10_000_000, **ABALONE)
    assert (fit.return_codes == 0).all()
    assert np.allclose(fit.lambda_, ref["lambda"], rtol=1e-12)
    scale = np.abs(ref["beta"]).max()
    err = np.abs(fit.beta - ref["beta"][0]).max() / scale
    print("abalone: covariance vs oracle, max coefficient difference / max|beta| = %.3g" % err)
    assert err <= ORACLE_TOL
    # intercepts and deviances below lambda_max only: there the oracle's stopping rule (coefficients only, all zero) leaves
    # ITS intercept short of mean(y), while this fit returns mean(y) itself
    assert abs(fit.a0[0] - ab["y"].mean()) <= 1e-12 * ab["y"].mean()
    assert np.abs(fit.a0[1:] - ref["a0"][0, 1:]).max() <= ORACLE_TOL * max(1.0, np.abs(ref["a0"]).max())
    assert np.abs(fit.dev_ratio[1:] - ref["dev_ratio"][1:]).max() <= ORACLE_TOL
    assert_optimal(sa.kkt(fit, ab["x"], ab["y"]), fit.lambda_, "abalone")


# ---- (iii) degenerate columns ----

def test_all_zero_sparse_column(sa):
    x, y = problem(120, 6, True, seed=3)
    x = sp.csc_matrix(sp.hstack([x[:, :2], sp.csc_matrix((120, 1)), x[:, 3:]]))
    for mix in (0.0, 1.0):
        fit = sa.sgdnet(x, y, alpha=mix, nlambda=8, lambda_min_ratio=1e-2, thresh=1e-12, maxit=100000, mode="covariance")
        assert (fit.beta[2] == 0.0).all() and (fit.return_codes == 0).all()
        assert_optimal(sa.kkt(fit, x, y), fit.lambda_, ("zero column", mix))


def test_constant_dense_column(sa):
    x, y = problem(120, 6, False, seed=4)
    x[:, 4] = 3.0
    for mix in (0.0, 1.0):
        for standardize in (True, False):
            fit = sa.sgdnet(x, y, alpha=mix, nlambda=8, lambda_min_ratio=1e-2, thresh=1e-12, maxit=100000, standardize=standardize,
                            mode="covariance")
            assert (fit.beta[4] == 0.0).all() and (fit.return_codes == 0).all() and np.isfinite(fit.beta).all()
            assert_optimal(sa.kkt(fit, x, y, standardize=standardize), fit.lambda_, ("constant column", mix, standardize))


def test_two_identical_columns_lasso(sa):
    x, y = problem(120, 6, False, seed=5)
    x[:, 5] = x[:, 1]
    fit = sa.sgdnet(x, y, alpha=1.0, nlambda=8, lambda_min_ratio=1e-2, thresh=1e-12, maxit=100000, mode="covariance")
    assert (fit.return_codes == 0).all() and np.isfinite(fit.beta).all()
    assert_optimal(sa.kkt(fit, x, y), fit.lambda_, "identical columns")


@pytest.mark.parametrize("sparse", [False, True])
def test_constant_response(sa, sparse):
    x, _ = problem(50, 4, sparse, seed=6)
    fit = sa.sgdnet(x, np.full(50, 2.5), alpha=0.5, nlambda=5, thresh=1e-12, mode="covariance")
    assert fit.nulldev == 0.0 and (fit.beta == 0.0).all() and not np.isnan(fit.dev_ratio).any()
    assert (fit.a0 == 2.5).all() and (fit.return_codes == 0).all()


# ---- (iv) cancellation: |mean| >> sd ----

@pytest.mark.parametrize("sparse", [False, True])
def test_large_mean_column_does_not_cancel(sa, sparse):
    x, y = problem(200, 5, sparse, seed=7)
    rng = np.random.default_rng(11)
    col = rng.standard_normal(200)
    col = (col - col.mean()) / col.std()                      # sd 1; the column below has mean 1e6 (every entry stored)
    xd = np.asarray(x.todense()) if sparse else x.copy()
    y = y + 0.7 * col
    shifted, centred = xd.copy(), xd.copy()
    shifted[:, 2], centred[:, 2] = 1e6 + col, col
    kw = dict(alpha=0.5, nlambda=10, lambda_min_ratio=0.05, thresh=1e-12, maxit=1_000_000, mode="covariance")
    wrap = sp.csc_matrix if sparse else np.asarray
    a, b = sa.sgdnet(wrap(shifted), y, **kw), sa.sgdnet(wrap(centred), y, **kw)
    assert (a.return_codes == 0).all()
    assert_optimal(sa.kkt(a, wrap(shifted), y), a.lambda_, ("mean 1e6", sparse))
    scale = np.abs(b.beta).max()
    print("mean 1e6 vs centred: max coefficient difference / max|beta| = %.3g" % (np.abs(a.beta - b.beta).max() / scale))
    assert np.abs(a.lambda_ - b.lambda_).max() <= ORACLE_TOL * b.lambda_.max()
    assert np.abs(a.beta - b.beta).max() <= ORACLE_TOL * scale
    assert np.abs(a.dev_ratio - b.dev_ratio).max() <= ORACLE_TOL


# ---- (v) determinism and the generator ----

@pytest.mark.parametrize("sparse", [False, True])
def test_bitwise_repeatable_and_draws_nothing(sa, sparse):
    x, y = problem(1003, 33, sparse, seed=8)
    rng = sa.RRng(3)
    before = bytes(rng.state)
    kw = dict(alpha=0.5, nlambda=10, lambda_min_ratio=1e-2, thresh=1e-9, maxit=100000, mode="covariance")
    a = sa.sgdnet(x, y, rng=rng, **kw)
    b = sa.sgdnet(x, y, seed=99, **kw)
    assert bytes(rng.state) == before
    assert a.beta.tobytes() == b.beta.tobytes() and a.a0.tobytes() == b.a0.tobytes()
    assert a.dev_ratio.tobytes() == b.dev_ratio.tobytes()
    assert a.draws_used == 0 and b.draws_used == 0 and a.npasses == b.npasses > 0


# ---- (vi) refusals ----

def refused(sa, needle, x, y, **kw):
    with pytest.raises(sa.SgdnetError) as e:
        sa.sgdnet(x, y, mode="covariance", **kw)
    assert e.value.code == -5, str(e.value)                   # SGDNET_EUNSUPPORTED
    assert "mode = covariance needs" in str(e.value) and needle in str(e.value), str(e.value)


def test_refusals_name_the_condition(sa):
    rng = np.random.default_rng(0)
    x = rng.standard_normal((60, 4))
    y = x[:, 0] + rng.standard_normal(60)
    wide = rng.standard_normal((20, pmax() + 1))
    refused(sa, "features (limit %d)" % pmax(), wide, wide[:, 0], nlambda=3)
    refused(sa, "sgdnet_covariance_max_features", sp.csc_matrix(wide), wide[:, 0], nlambda=3)
    refused(sa, "family = gaussian", x, (y > 0).astype(float), family="binomial", nlambda=3)
    refused(sa, "family = gaussian", x, np.column_stack([y, -y]), family="mgaussian", nlambda=3)
    refused(sa, "one GPU", x, y, nlambda=3, devices=[0, 0])
    refused(sa, "one GPU", sp.csc_matrix(x), y, nlambda=3, devices=[0, 0])
    refused(sa, "debug = 0", x, y, nlambda=3, debug=True)
    # ... and no other mode reaches the solver: the SAGA modes still draw
    assert sa.sgdnet(x, y, nlambda=3, mode="auto").draws_used > 0


# ---- (vii) the R shim ----

@pytest.mark.parametrize("sparse", [False, True])
def test_shim_option_gives_the_ctypes_fit(sa, sparse):
    import rshim
    R = rshim.lib()
    R.rmock_reset()
    R.R_init_sgdnet(None)
    n, p, nl = 300, 6, 12
    x, y = problem(n, p, sparse, seed=9)
    rshim.set_option("sgdnet.mode", "covariance")
    R.rmock_set_seed(7)
    ctl = rshim.control_list(family="gaussian", alpha=0.5, nlambda=nl, lambda_min_ratio=1e-3, thresh=1e-9, maxit=100000,
                             is_sparse=sparse)
    got = rshim.decode_result(rshim.call("_sgdnet_SgdnetSparse" if sparse else "_sgdnet_SgdnetDense",
                                         rshim.r_dgcmatrix(x) if sparse else rshim.r_matrix(x), rshim.r_matrix(y.reshape(n, 1)), ctl))
    ref = sa.sgdnet(x, y, alpha=0.5, nlambda=nl, lambda_min_ratio=1e-3, thresh=1e-9, maxit=100000, mode="covariance")
    assert got["unlist_beta"].tobytes() == ref.beta.ravel(order="F").tobytes()
    assert got["a0"][0].tobytes() == ref.a0.tobytes() and got["lambda_"].tobytes() == ref.lambda_.tobytes()
    assert got["dev_ratio"].tobytes() == ref.dev_ratio.tobytes() and got["npasses"] == ref.npasses
    assert R.rmock_unif_count() == 0 and R.rmock_protect_depth() == 0
