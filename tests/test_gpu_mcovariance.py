"""sa.sgdnet_mcovariance (SGDNET_MODE_MCOVARIANCE, sgdnet_amd/csrc/covariance.hip: cov_group_path_kernel): the mgaussian
path of K responses solved to its optimum from the device's centred X'X and X'Y by block coordinate descent.  Checked
against the optimality conditions of the problem the driver solves (sa.kkt: device gradient on the data as it came + the
numpy conventions of sgdnet_amd/kkt.py); the shapes sit at the kernels' edges (one stride of the workgroup over the
p K entries, the column tiles of the moments pass with the responses across a tile edge, one workgroup's LDS).

mix = 0.5 -- the group lasso with a ridge part -- is the case no other mode solves: the reference's iteration has no
fixed point there (tests/test_kkt_host.py), so there is no oracle to compare with and the certificate is the check.

numpy_block_cd_path() and numpy_kkt() below restate the algorithm and the certificate in numpy;
tests/test_mcovariance_host.py checks on the CPU that the restatement's optimum stays inside the bound used here for
the same inputs, and measures the oracle's distance from its own optimum (ORACLE_* below).

Seen on an MI355X: worst KKT ratio 2.3e-10 and intercept residual 1.6e-10 lambda (both at the column of mean 1e6; 1e-11
and below elsewhere), dev_ratio within 1e-15 of the residuals', the oracle cases at the oracle's own distance."""
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

# The project's optimality bound (tests/test_gpu_covariance.py, tests/test_gpu_parity.py): KKT residual <= 1e-8 * lambda.
KKT_BOUND = 1e-8
# dev_ratio against 1 - RSS / nulldev from the returned coefficients: the terms of the quadratic form are bounded by
# y'y and there are n + p K roundings (test_mcovariance_host.py shows the numpy quadratic form inside this)
DEV_TOL = 1e-10

# (n, p, K); p = None: sa.mcovariance_max_features(K)
SMALL_SHAPES = [(5, 1, 2), (37, 2, 3), (63, 16, 4), (65, 13, 5), (1003, 33, 3)]
LIMIT_SHAPES = [(300, None, 2), (300, None, 10)]
SETTINGS = [(True, True), (True, False), (False, True), (False, False)]      # (intercept, standardize)
NONMONOTONE = [0.3, 0.02, 0.8, 0.1, 0.05]
PATH = dict(nlambda=20, lambda_min_ratio=1e-2, thresh=1e-12, maxit=1_000_000)

# The CPU oracle (SAGA) has an optimum to converge to at mix = 1 and mix = 0.  On oracle_problem(), per case (mix,
# standardize_response): the largest change of its own coefficients between thresh = 1e-9 and thresh = 1e-11, relative
# to max|beta| -- its distance from the optimum at 1e-9 -- and the same for its intercepts from the second lambda on,
# relative to max(1, max|a0|).  Measured and pinned by test_mcovariance_host.py::test_oracle_distance_from_its_optimum;
# the tolerances are 10 x these.
ORACLE_THRESH = 1e-9
ORACLE_PATH = dict(nlambda=10, lambda_min_ratio=1e-2)
ORACLE_CASES = [(1.0, False), (1.0, True), (0.0, False), (0.0, True)]
ORACLE_REL_CHANGE = {(1.0, False): 1.01e-9, (1.0, True): 6.5e-10, (0.0, False): 4.6e-10, (0.0, True): 3.7e-10}     # measured 1.00e-9, 6.43e-10, 4.58e-10, 3.63e-10
ORACLE_A0_CHANGE = {(1.0, False): 3.5e-9, (1.0, True): 1.1e-9, (0.0, False): 8.2e-8, (0.0, True): 9.8e-9}          # measured 3.43e-9, 1.06e-9, 8.13e-8, 9.73e-9
# the tolerance of the one-response cancellation test (tests/test_gpu_covariance.py: ORACLE_TOL)
CANCEL_TOL = 10 * 8.3e-9


def pmax(K):
    import sgdnet_amd as sa
    return sa.mcovariance_max_features(K)


def problem(n, p, K, sparse, seed=0):
    """x with columns of different means and scales (sparse: ~35 % stored, the first row always), y = x B + noise with
    half of B's rows zero and a different mean per response."""
    rng = np.random.default_rng(1000 * seed + 7 * n + 31 * p + K)
    x = rng.standard_normal((n, p)) * rng.uniform(0.5, 3.0, p) + rng.uniform(-2.0, 2.0, p)
    if sparse:
        keep = rng.random((n, p)) < 0.35
        keep[0, :] = True
        x = x * keep
    B = rng.standard_normal((p, K)) * (rng.random(p) < 0.5)[:, None]
    y = x @ B + 0.5 * rng.standard_normal((n, K)) * rng.uniform(0.5, 2.0, K) + rng.uniform(-2.0, 2.0, K)
    return (sp.csc_matrix(x) if sparse else x), y


def oracle_problem():
    return problem(200, 6, 3, False, seed=20)


def dense(x):
    return np.asarray(x.todense()) if sp.issparse(x) else np.asarray(x, dtype=float)


def preprocessed_response(y, standardize_response):
    """prepare_response (driver.cpp) for mgaussian: standardised only on request, and then the fit stays on that scale."""
    y = np.asarray(y, dtype=float)
    if not standardize_response:
        return y
    sd = y.std(axis=0)
    return (y - y.mean(axis=0)) / np.where(sd == 0, 1.0, sd)


def numpy_block_cd_path(x, y, lam, mix, standardize=True, intercept=True, standardize_response=False, tol=1e-13, max_sweeps=200000):
    """Cyclic block coordinate descent with covariance updates in the driver's units (sgdnet_amd/kkt.py):
    (a0 (K, L), beta (K, p, L), dev_ratio (L) from the quadratic form)."""
    x, y = dense(x), preprocessed_response(y, standardize_response)
    n, p = x.shape
    K = y.shape[1]
    b0 = y.mean(axis=0)
    mean = x.mean(axis=0)
    var = ((x - mean) ** 2).mean(axis=0)
    sd = np.where(var == 0, 1.0, np.sqrt(var)) if standardize else np.ones(p)
    mu = mean if (standardize or intercept) else np.zeros(p)
    xt, yt = (x - mu) / sd, y - b0
    S, c = xt.T @ xt / n, xt.T @ yt / n
    yy, nulldev = (yt ** 2).sum(), ((y - y.mean(axis=0)) ** 2).sum()
    w = np.zeros((p, K))
    a0, beta, dev_ratio = [], [], []
    for l in lam:
        l1, l2 = mix * l, (1 - mix) * l
        g = S @ w - c
        for _ in range(max_sweeps):
            change = 0.0
            for j in range(p):
                z, den = S[j, j] * w[j] - g[j], S[j, j] + l2
                nz = np.sqrt((z * z).sum())
                if nz == 0.0 or den <= 0.0:
                    nw = np.zeros(K)
                else:
                    nw = (1.0 if mix == 0 else max(0.0, 1.0 - l1 / nz)) * z / den
                d = nw - w[j]
                if d.any():
                    w[j] = nw
                    g += np.outer(S[:, j], d)
                    change = max(change, np.abs(d).max())
            if change <= tol * np.abs(w).max():
                break
        b = w / sd[:, None]
        beta.append(b.T.copy())
        a0.append(b0 - mean @ b if intercept else b0.copy())
        dev_ratio.append(1.0 - (yy - n * (w * (c - g)).sum()) / nulldev if nulldev > 0 else 0.0)
    return np.array(a0).T, np.moveaxis(np.array(beta), 0, 2), np.array(dev_ratio)


def as_fit(a0, beta, lam, mix):
    return SimpleNamespace(a0=np.asarray(a0), beta=np.asarray(beta), lambda_=np.asarray(lam, dtype=float), alpha=mix, family="mgaussian")


def stacked(fit):
    return np.stack([np.asarray(b) for b in fit.beta])              # (K, p, L)


def numpy_kkt(a0, beta, x, y, lam, mix, standardize, intercept, standardize_response=False):
    """sa.kkt without the device: the gradient of the gaussian loss of every response in numpy, then kkt_from_gradient."""
    import sgdnet_amd as sa
    fit = as_fit(a0, beta, lam, mix)
    xc, xs = sa.feature_moments(x, standardize)
    xd, yd = dense(x), preprocessed_response(y, standardize_response)
    ev = sa.evaluation_intercepts(fit, xc, None, intercept)                         # (K, L)
    r = ev[None] + np.einsum("ij,kjl->ikl", xd, fit.beta) - yd[:, :, None]          # (n, K, L)
    G, G0 = np.einsum("ij,ikl->kjl", xd, r) / len(yd), r.mean(axis=0)
    return sa.kkt_from_gradient(G, G0, fit, x_center=xc, x_scale=xs, y_scale=None, standardize=standardize, intercept=intercept)


def numpy_dev_ratio(a0, beta, x, y, standardize, intercept, standardize_response=False):
    """1 - RSS / nulldev of the preprocessed response at the predictor the driver fits (kkt.py: evaluation_intercepts)."""
    import sgdnet_amd as sa
    xc, _ = sa.feature_moments(x, standardize)
    xd, yd = dense(x), preprocessed_response(y, standardize_response)
    ev = sa.evaluation_intercepts(SimpleNamespace(a0=np.asarray(a0), beta=np.asarray(beta)), xc, None, intercept)
    r = ev[None] + np.einsum("ij,kjl->ikl", xd, np.asarray(beta)) - yd[:, :, None]
    nulldev = ((yd - yd.mean(axis=0)) ** 2).sum()
    return 1.0 - (r ** 2).sum(axis=(0, 1)) / nulldev


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


def check_fit(sa, fit, x, y, what, standardize=True, intercept=True, standardize_response=False):
    assert (fit.return_codes == 0).all() and fit.draws_used == 0 and np.isfinite(fit.dev_ratio).all(), what
    k = sa.kkt(fit, x, y, standardize=standardize, intercept=intercept, standardize_response=standardize_response)
    assert_optimal(k, fit.lambda_, what)                                            # no lambda dropped
    ref = numpy_dev_ratio(fit.a0, stacked(fit), x, y, standardize, intercept, standardize_response)
    print(what, "dev_ratio vs numpy max %.3g" % np.abs(fit.dev_ratio - ref).max())
    assert np.abs(fit.dev_ratio - ref).max() <= DEV_TOL, what


# ---- (i) optimality and deviance across the envelope ----

@pytest.mark.parametrize("mix", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", SMALL_SHAPES)
def test_automatic_path_is_optimal(sa, shape, sparse, mix):
    n, p, K = shape
    x, y = problem(n, p, K, sparse)
    for intercept, standardize in SETTINGS:
        fit = sa.sgdnet_mcovariance(x, y, alpha=mix, intercept=intercept, standardize=standardize, **PATH)
        check_fit(sa, fit, x, y, (n, p, K, sparse, mix, intercept, standardize), standardize, intercept)


@pytest.mark.parametrize("mix", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", LIMIT_SHAPES)
def test_path_at_the_feature_limit_is_optimal(sa, shape, sparse, mix):
    n, K = shape[0], shape[2]
    p = pmax(K)
    x, y = problem(n, p, K, sparse)
    for intercept, standardize in SETTINGS:
        fit = sa.sgdnet_mcovariance(x, y, alpha=mix, intercept=intercept, standardize=standardize, **dict(PATH, nlambda=4))
        check_fit(sa, fit, x, y, (n, p, K, sparse, mix, intercept, standardize), standardize, intercept)


@pytest.mark.parametrize("mix", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("sparse", [False, True])
def test_standardized_response(sa, sparse, mix):
    x, y = problem(65, 13, 5, sparse, seed=1)
    fit = sa.sgdnet_mcovariance(x, y, alpha=mix, standardize_response=True, **PATH)
    check_fit(sa, fit, x, y, ("standardize_response", sparse, mix), standardize_response=True)


@pytest.mark.parametrize("sparse", [False, True])
def test_user_lambdas_need_not_be_monotone(sa, sparse):
    x, y = problem(65, 13, 5, sparse, seed=2)
    kw = dict(alpha=0.5, thresh=1e-12, maxit=1_000_000)
    fit = sa.sgdnet_mcovariance(x, y, lambda_=NONMONOTONE, **kw)
    assert np.array_equal(fit.lambda_, NONMONOTONE)
    check_fit(sa, fit, x, y, ("user lambdas", sparse))
    # every lambda's optimum is its own: the same values in decreasing order give the same coefficients
    order = np.argsort(NONMONOTONE)[::-1]
    mono = sa.sgdnet_mcovariance(x, y, lambda_=np.array(NONMONOTONE)[order], **kw)
    assert np.abs(stacked(fit)[:, :, order] - stacked(mono)).max() <= 1e-9 * np.abs(stacked(mono)).max()


def test_max_iter_is_reported(sa):
    x, y = problem(65, 13, 5, False, seed=3)
    fit = sa.sgdnet_mcovariance(x, y, alpha=0.5, nlambda=5, lambda_min_ratio=1e-2, thresh=1e-14, maxit=2)
    assert (fit.return_codes[1:] == 1).all() and 2 * 4 + 1 <= fit.npasses <= 2 * 5


# ---- (ii) the same lambdas as, and the same optimum as, the existing solvers ----

@pytest.mark.parametrize("standardize_response", [False, True])
def test_same_lambdas_and_null_deviance_as_exact_mode(sa, standardize_response):
    x, y = oracle_problem()
    kw = dict(alpha=0.5, nlambda=12, lambda_min_ratio=1e-2, standardize_response=standardize_response)
    new = sa.sgdnet_mcovariance(x, y, **kw)
    exact = sa.sgdnet(x, y, family="mgaussian", mode="exact", **kw)
    assert new.lambda_.tobytes() == exact.lambda_.tobytes() and new.nulldev == exact.nulldev


@pytest.mark.parametrize("case", ORACLE_CASES)
def test_same_optimum_as_the_oracle(sa, oracle, case):
    mix, standardize_response = case
    x, y = oracle_problem()
    kw = dict(alpha=mix, standardize_response=standardize_response, **ORACLE_PATH)
    ref = oracle.fit(x, y, family="mgaussian", thresh=ORACLE_THRESH, maxit=100000, seed=1, **kw)
    fit = sa.sgdnet_mcovariance(x, y, thresh=1e-12, maxit=1_000_000, **kw)
    assert (fit.return_codes == 0).all() and (ref["return_codes"] == 0).all()
    assert np.allclose(fit.lambda_, ref["lambda"], rtol=1e-12, atol=0)
    tol, a0_tol = 10 * ORACLE_REL_CHANGE[case], 10 * ORACLE_A0_CHANGE[case]
    err = np.abs(stacked(fit) - ref["beta"]).max() / np.abs(ref["beta"]).max()
    # intercepts and deviances from the second lambda on: at lambda_max the oracle's stopping rule (coefficients only, all
    # zero) leaves ITS intercept short of the mean
    a0_err = np.abs(fit.a0[:, 1:] - ref["a0"][:, 1:]).max() / max(1.0, np.abs(ref["a0"]).max())
    dev_err = np.abs(fit.dev_ratio[1:] - ref["dev_ratio"][1:]).max()
    print(case, "vs oracle: coefficients %.3g (tol %.3g) intercepts %.3g (tol %.3g) dev_ratio %.3g" % (err, tol, a0_err, a0_tol, dev_err))
    assert err <= tol
    assert a0_err <= a0_tol
    assert dev_err <= tol
    check_fit(sa, fit, x, y, ("oracle problem", case), standardize_response=standardize_response)


# ---- (iii) degenerate inputs ----

def test_all_zero_sparse_column(sa):
    x, y = problem(120, 6, 3, True, seed=4)
    x = sp.csc_matrix(sp.hstack([x[:, :2], sp.csc_matrix((120, 1)), x[:, 3:]]))
    for mix in (0.0, 0.5, 1.0):
        fit = sa.sgdnet_mcovariance(x, y, alpha=mix, nlambda=8, lambda_min_ratio=1e-2, thresh=1e-12, maxit=100000)
        assert (stacked(fit)[:, 2] == 0.0).all()
        check_fit(sa, fit, x, y, ("zero column", mix))


def test_constant_dense_column(sa):
    x, y = problem(120, 6, 3, False, seed=5)
    x[:, 4] = 3.0
    for mix in (0.0, 0.5, 1.0):
        for standardize in (True, False):
            fit = sa.sgdnet_mcovariance(x, y, alpha=mix, nlambda=8, lambda_min_ratio=1e-2, thresh=1e-12, maxit=100000,
                                        standardize=standardize)
            assert (stacked(fit)[:, 4] == 0.0).all() and np.isfinite(stacked(fit)).all()
            check_fit(sa, fit, x, y, ("constant column", mix, standardize), standardize=standardize)


def test_two_identical_columns_group_lasso(sa):
    x, y = problem(120, 6, 3, False, seed=6)
    x[:, 5] = x[:, 1]
    fit = sa.sgdnet_mcovariance(x, y, alpha=1.0, nlambda=8, lambda_min_ratio=1e-2, thresh=1e-12, maxit=100000)
    assert np.isfinite(stacked(fit)).all()
    check_fit(sa, fit, x, y, "identical columns")


@pytest.mark.parametrize("sparse", [False, True])
def test_one_constant_response_among_varying_ones(sa, sparse):
    x, y = problem(120, 6, 3, sparse, seed=7)
    y[:, 1] = -4.25
    for mix in (0.0, 0.5, 1.0):
        fit = sa.sgdnet_mcovariance(x, y, alpha=mix, nlambda=8, lambda_min_ratio=1e-2, thresh=1e-12, maxit=100000)
        assert (stacked(fit)[1] == 0.0).all() and (fit.a0[1] == -4.25).all()
        check_fit(sa, fit, x, y, ("constant response column", sparse, mix))


@pytest.mark.parametrize("sparse", [False, True])
def test_all_responses_constant(sa, sparse):
    x, _ = problem(50, 4, 3, sparse, seed=8)
    y = np.tile([2.5, -1.0, 0.0], (50, 1))
    fit = sa.sgdnet_mcovariance(x, y, alpha=0.5, nlambda=5, thresh=1e-12)
    assert fit.nulldev == 0.0 and (stacked(fit) == 0.0).all() and not np.isnan(fit.dev_ratio).any()
    assert (fit.a0 == y[0][:, None]).all() and (fit.return_codes == 0).all()


# ---- (iv) cancellation: |mean| >> sd ----

@pytest.mark.parametrize("sparse", [False, True])
def test_large_mean_column_does_not_cancel(sa, sparse):
    x, y = problem(200, 5, 3, sparse, seed=9)
    rng = np.random.default_rng(11)
    col = rng.standard_normal(200)
    col = (col - col.mean()) / col.std()                      # sd 1; the column below has mean 1e6 (every entry stored)
    xd = dense(x).copy()
    y = y + np.outer(col, [0.7, -0.4, 0.2])
    shifted, centred = xd.copy(), xd.copy()
    shifted[:, 2], centred[:, 2] = 1e6 + col, col
    kw = dict(alpha=0.5, nlambda=10, lambda_min_ratio=0.05, thresh=1e-12, maxit=1_000_000)
    wrap = sp.csc_matrix if sparse else np.asarray
    a, b = sa.sgdnet_mcovariance(wrap(shifted), y, **kw), sa.sgdnet_mcovariance(wrap(centred), y, **kw)
    assert (a.return_codes == 0).all()
    assert_optimal(sa.kkt(a, wrap(shifted), y), a.lambda_, ("mean 1e6", sparse))
    scale = np.abs(stacked(b)).max()
    print("mean 1e6 vs centred: max coefficient difference / max|beta| = %.3g" % (np.abs(stacked(a) - stacked(b)).max() / scale))
    assert np.abs(a.lambda_ - b.lambda_).max() <= CANCEL_TOL * b.lambda_.max()
    assert np.abs(stacked(a) - stacked(b)).max() <= CANCEL_TOL * scale
    assert np.abs(a.dev_ratio - b.dev_ratio).max() <= CANCEL_TOL


# ---- (v) determinism and the generator ----

@pytest.mark.parametrize("sparse", [False, True])
def test_bitwise_repeatable_and_draws_nothing(sa, sparse):
    x, y = problem(1003, 33, 3, sparse, seed=10)
    rng = sa.RRng(3)
    before = bytes(rng.state)
    kw = dict(alpha=0.5, nlambda=10, lambda_min_ratio=1e-2, thresh=1e-9, maxit=100000)
    a = sa.sgdnet_mcovariance(x, y, **kw)
    b = sa.sgdnet_mcovariance(x, y, **kw)
    assert bytes(rng.state) == before
    assert stacked(a).tobytes() == stacked(b).tobytes() and a.a0.tobytes() == b.a0.tobytes()
    assert a.dev_ratio.tobytes() == b.dev_ratio.tobytes()
    assert a.draws_used == 0 and b.draws_used == 0 and a.npasses == b.npasses > 0
    # a generator the caller holds is not advanced by the backend either: mode 5 through the native entry with rng_state set
    from sgdnet_amd import _lib, api
    c = api._fit(x, y, "mgaussian", 0.5, 10, 1e-2, None, 100000, True, True, 1e-9, False, debug=False, seed=0, rng=rng,
                 sample_stream=None, unif=None, mode="mcovariance", modes={"mcovariance": _lib.MODE_MCOVARIANCE}, batch=0, device=0,
                 devices=None)
    assert bytes(rng.state) == before and stacked(c).tobytes() == stacked(a).tobytes()


# ---- (vi) refusals ----

def refused(sa, needle, x, y, family="mgaussian", **kw):
    from sgdnet_amd import _lib, api
    args = dict(debug=False, seed=0, rng=None, sample_stream=None, unif=None, batch=0, device=0, devices=None)
    args.update(kw)
    with pytest.raises(sa.SgdnetError) as e:
        api._fit(x, y, family, 0.5, 3, None, None, 1000, True, True, 1e-3, False, mode="mcovariance",
                 modes={"mcovariance": _lib.MODE_MCOVARIANCE}, **args)
    assert e.value.code == -5, str(e.value)                   # SGDNET_EUNSUPPORTED
    assert "mode = mcovariance needs " in str(e.value) and needle in str(e.value), str(e.value)


def test_refusals_name_the_condition(sa):
    rng = np.random.default_rng(0)
    x = rng.standard_normal((60, 4))
    y = np.column_stack([x[:, 0] + rng.standard_normal(60), x[:, 1] - rng.standard_normal(60)])
    for K in (2, 10):
        wide = rng.standard_normal((20, pmax(K) + 1))
        yk = rng.standard_normal((20, K))
        refused(sa, "features (limit %d)" % pmax(K), wide, yk)
        refused(sa, "sgdnet_mcovariance_max_features(n_classes)", sp.csc_matrix(wide), yk)
        with pytest.raises(sa.SgdnetError, match="mode = mcovariance needs no more features"):
            sa.sgdnet_mcovariance(wide, yk, nlambda=3)
        assert sa.sgdnet_mcovariance(wide[:, :-1], yk, nlambda=3, lambda_min_ratio=0.5).draws_used == 0      # the limit itself is taken
    refused(sa, "family = mgaussian", x, y[:, 0], family="gaussian")
    refused(sa, "family = mgaussian", x, (y[:, 0] > 0).astype(float), family="binomial")
    refused(sa, "one GPU", x, y, devices=[0, 0])
    refused(sa, "one GPU", sp.csc_matrix(x), y, devices=[0, 0])
    refused(sa, "debug = 0", x, y, debug=True)


def test_the_other_doors_stay_shut(sa):
    rng = np.random.default_rng(1)
    x = rng.standard_normal((60, 4))
    y = np.column_stack([x[:, 0] + rng.standard_normal(60), x[:, 1] - rng.standard_normal(60)])
    with pytest.raises(ValueError, match="mode must be one of"):
        sa.sgdnet(x, y, family="mgaussian", nlambda=3, mode="mcovariance")
    with pytest.raises(sa.SgdnetError) as e:
        sa.sgdnet(x, y, family="mgaussian", nlambda=3, mode="covariance")
    assert e.value.code == -5 and "mode = covariance needs family = gaussian" in str(e.value)
    # ... and no other mode reaches the solver: the SAGA modes still draw
    assert sa.sgdnet(x, y, family="mgaussian", nlambda=3, mode="auto").draws_used > 0
    assert sa.sgdnet_mcovariance(x, y, nlambda=3).draws_used == 0


# ---- (vii) the R shim ----

@pytest.mark.parametrize("sparse", [False, True])
def test_shim_option_gives_the_ctypes_fit(sa, sparse):
    import rshim
    R = rshim.lib()
    R.rmock_reset()
    R.R_init_sgdnet(None)
    n, p, K, nl = 300, 6, 2, 12
    x, y = problem(n, p, K, sparse, seed=12)
    rshim.set_option("sgdnet.mode", "mcovariance")
    R.rmock_set_seed(7)
    kw = dict(alpha=0.5, nlambda=nl, lambda_min_ratio=1e-3, thresh=1e-9, maxit=100000)
    ctl = rshim.control_list(family="mgaussian", n_classes=K, is_sparse=sparse, **kw)
    got = rshim.decode_result(rshim.call("_sgdnet_SgdnetSparse" if sparse else "_sgdnet_SgdnetDense",
                                         rshim.r_dgcmatrix(x) if sparse else rshim.r_matrix(x), rshim.r_matrix(y), ctl))
    ref = sa.sgdnet_mcovariance(x, y, **kw)
    assert got["unlist_beta"].tobytes() == stacked(ref).ravel(order="F").tobytes()
    assert np.asfortranarray(got["a0"]).tobytes(order="F") == np.asfortranarray(ref.a0).tobytes(order="F")
    assert got["lambda_"].tobytes() == ref.lambda_.tobytes()
    assert got["dev_ratio"].tobytes() == ref.dev_ratio.tobytes() and got["npasses"] == ref.npasses
    assert R.rmock_unif_count() == 0 and R.rmock_protect_depth() == 0
