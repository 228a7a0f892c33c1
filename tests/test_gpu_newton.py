"""sa.sgdnet_newton (SGDNET_MODE_NEWTON, sgdnet_amd/csrc/newton.hip): the binomial path of one response solved to its
optimum by proximal Newton steps on the device.  Checked against the optimality conditions of the problem the driver
solves (sa.kkt: device gradient on the data as it came + the numpy conventions of sgdnet_amd/kkt.py), not against
another solver's iterates; the shapes put p + 1 and p + 2 on both sides of the 16-column tile, n on both sides of the
64-row step, and one at the limit of one workgroup's LDS.

numpy_newton_path() below restates the algorithm in numpy; tests/test_newton_host.py checks on the CPU that this
restatement reproduces scikit-learn and that its optimum stays inside the bound used here for the same inputs."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp

import test_gpu_covariance as tc

pytestmark = pytest.mark.gpu
GOLD = tc.GOLD

# The project's optimality bound (tests/test_gpu_covariance.py, tests/test_gpu_parity.py): KKT residual <= 1e-8 * lambda,
# for the coefficients and for the intercept.
KKT_BOUND = tc.KKT_BOUND
# Coefficient tolerance against the CPU oracle (SAGA at thresh = 1e-9) on the binomial abalone path of
# test_same_optimum_as_the_oracle_on_abalone, relative to max|beta|: 10 x the oracle's own change between thresh = 1e-9
# and thresh = 1e-11, measured 6.31e-9 (its distance from the optimum at that thresh; the measurement is
# test_newton_host.py::test_oracle_distance_from_its_optimum_on_abalone).
ORACLE_REL_CHANGE = 6.4e-9
ORACLE_TOL = 10 * ORACLE_REL_CHANGE
ABALONE = dict(alpha=0.5, nlambda=12, lambda_min_ratio=1e-2)
ORACLE_THRESH = 1e-9

SHAPES = [(40, 1), (37, 2), (63, 14), (65, 15), (65, 16), (1003, 33), (600, None)]     # None: sgdnet_newton_max_features()
SETTINGS = [(True, True), (True, False), (False, True), (False, False)]                # (intercept, standardize)
NLAMBDA, THRESH = 12, 1e-12
NONMONOTONE = [0.03, 0.002, 0.08, 0.01, 0.005]
# the constants of csrc/newton.hpp, restated for numpy_newton_path
MAX_HALVINGS, OBJECTIVE_SLACK, MAX_SWEEPS, NEGLIGIBLE = 10, 1e-12, 1000, 16 * 2.220446049250313e-16


def pmax():
    import sgdnet_amd as sa
    return sa.newton_max_features()


def ratio_for(p):
    return 5e-2 if p == pmax() else 1e-2


def problem(n, p, sparse, seed=0):
    """x as test_gpu_covariance.problem makes it; class labels drawn from the logistic model with coefficients B / sqrt(p / 4)
    on the centred columns."""
    x, _ = tc.problem(n, p, sparse, seed)
    xd = np.asarray(x.todense()) if sparse else x
    rng = np.random.default_rng(5000 * seed + 11 * n + p)
    B = rng.standard_normal(p) * (rng.random(p) < 0.5) / np.sqrt(p / 4)
    eta = (xd - xd.mean(axis=0)) @ B + 0.3
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-eta))).astype(float)
    assert min(y.sum(), n - y.sum()) >= 2
    return x, y


def abalone_binomial():
    ab = np.load(os.path.join(GOLD, "abalone.npz"))
    return ab["x"], (ab["y"] > np.median(ab["y"])).astype(float)


def automatic_lambdas(x, y, mix, standardize, nlambda, ratio):
    """regularization_path / lambda_max of the driver for a binomial response (driver.cpp)."""
    import sgdnet_amd as sa
    xd = np.asarray(x.todense()) if sp.issparse(x) else x
    xc, xs = sa.feature_moments(x, standardize)
    lmax = np.abs(((xd - xc) / xs).T @ (y - y.mean())).max() / len(y) / max(mix, 0.001)
    return np.exp(np.linspace(np.log(lmax), np.log(lmax * ratio), nlambda))


def numpy_newton_path(x, y, lam, mix, standardize=True, intercept=True, thresh=THRESH, maxit=1000):
    """The algorithm of csrc/newton.hip in numpy, in the driver's units (sgdnet_amd/kkt.py): per outer step the state
    (mu, v, r, loss) at the iterate, the weighted moments H and q of [x - m | 1] / s, cyclic coordinate descent on the
    penalised quadratic model (the intercept last, unpenalised), halving while the objective rose.
    Returns (a0 (L,), beta (p, L), info)."""
    x = np.asarray(x.todense()) if sp.issparse(x) else np.asarray(x, dtype=float)
    n, p = x.shape
    mean = x.mean(axis=0)
    var = ((x - mean) ** 2).mean(axis=0)
    sd = np.where(var == 0, 1.0, np.sqrt(var)) if standardize else np.ones(p)
    m = mean if (standardize or intercept) else np.zeros(p)
    centre = mean if standardize else np.zeros(p)                 # the driver's x_center
    Z = np.column_stack([(x - m) / sd, np.ones(n)])
    ybar = min(max(y.mean(), 1e-9), 1 - 1e-9)
    u = np.zeros(p + 1)
    u[p] = np.log(ybar / (1 - ybar)) if intercept else 0.0
    n_coord = p + 1 if intercept else p

    def state(u):
        eta = Z @ u
        e = np.exp(eta)
        t = 1.0 / (1.0 + e)
        return t * (1 - t), t - (1 - y), (np.log(1 + e) - y * eta).mean()

    def penalty(u, l1, l2):
        return l2 * 0.5 * (u[:p] ** 2).sum() + l1 * np.abs(u[:p]).sum()

    v, r, loss = state(u)
    info = dict(halvings=0, steps=[], codes=[], passes=1)
    a0, beta = [], []
    for l in lam:
        l1, l2 = (0.0 if mix == 0 else mix * l), (1 - mix) * l
        objective = loss + penalty(u, l1, l2)
        steps, converged = 0, False
        while steps < maxit and not converged:
            H, q = (Z * v[:, None]).T @ Z / n, Z.T @ r / n
            c, g = u.copy(), -q.copy()
            inner = negligible = False
            for _ in range(MAX_SWEEPS):
                change = size = eta_sq = 0.0
                for j in range(n_coord):
                    z, den = H[j, j] * c[j] - g[j], H[j, j] + (l2 if j < p else 0.0)
                    nu = np.sign(z) * max(abs(z) - l1, 0.0) if (j < p and mix != 0) else z
                    nu = nu / den if den > 0 else (0.0 if j < p else c[j])
                    d = nu - c[j]
                    change, size, eta_sq = max(change, abs(d)), max(size, abs(nu)), max(eta_sq, nu * nu * H[j, j])
                    if d != 0.0:
                        c[j] = nu
                        g += H[:, j] * d
                negligible = eta_sq <= NEGLIGIBLE ** 2                  # zero to rounding (newton.hpp)
                if (size == 0 and change == 0) or (size != 0 and change / size <= thresh) or negligible:
                    inner = True
                    break
            v, r, cl = state(c)
            info["passes"] += 1
            candidate = cl + penalty(c, l1, l2)
            h = 0
            while h < MAX_HALVINGS and np.abs(c - u).max() > 0 and not candidate <= objective + OBJECTIVE_SLACK * abs(objective):
                c = u + 0.5 * (c - u)
                v, r, cl = state(c)
                info["passes"] += 1
                candidate = cl + penalty(c, l1, l2)
                h += 1
                negligible = False
            info["halvings"] += h
            change, size = np.abs(c - u).max(), np.abs(c).max()
            u, loss, objective = c, cl, candidate
            steps += 1
            converged = inner and ((size == 0 and change == 0) or (size != 0 and change / size <= thresh) or negligible)
        info["steps"].append(steps)
        info["codes"].append(0 if converged else 1)
        b = u[:p] / sd
        beta.append(b)
        a0.append(u[p] - (m - centre) @ b - centre @ b if intercept else 0.0)
    return np.array(a0), np.array(beta).T, info


def numpy_kkt(a0, beta, x, y, lam, mix, standardize, intercept):
    """sa.kkt without the device: the gradient of the binomial loss in numpy, then kkt_from_gradient."""
    import sgdnet_amd as sa
    fit = SimpleNamespace(a0=np.asarray(a0), beta=np.asarray(beta), lambda_=np.asarray(lam, dtype=float), alpha=mix, family="binomial")
    xc, xs = sa.feature_moments(x, standardize)
    yc, ysc = sa.response_moments(fit, y)
    xd = np.asarray(x.todense()) if sp.issparse(x) else np.asarray(x, dtype=float)
    ev = sa.evaluation_intercepts(fit, xc, yc, intercept)                       # (1, L)
    r = 1.0 - np.asarray(y, dtype=float)[:, None] - 1.0 / (1.0 + np.exp(ev + xd @ fit.beta))      # (n, L): families.h Gradient
    G, G0 = (xd.T @ r / len(y))[None], r.mean(axis=0)[None]
    return sa.kkt_from_gradient(G, G0, fit, x_center=xc, x_scale=xs, y_scale=ysc, standardize=standardize, intercept=intercept)


assert_optimal = tc.assert_optimal


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
    for intercept, standardize in SETTINGS:
        fit = sa.sgdnet_newton(x, y, alpha=mix, nlambda=NLAMBDA, lambda_min_ratio=ratio_for(p), thresh=THRESH, intercept=intercept,
                               standardize=standardize)
        assert fit.family == "binomial" and fit.beta.shape == (p, NLAMBDA)
        assert (fit.return_codes == 0).all() and fit.draws_used == 0 and np.isfinite(fit.dev_ratio).all()
        k = sa.kkt(fit, x, y, standardize=standardize, intercept=intercept)
        assert_optimal(k, fit.lambda_, (n, p, sparse, mix, intercept, standardize))     # no lambda dropped


@pytest.mark.parametrize("sparse", [False, True])
def test_user_lambdas_need_not_be_monotone(sa, sparse):
    x, y = problem(65, 16, sparse, seed=1)
    fit = sa.sgdnet_newton(x, y, alpha=0.5, lambda_=NONMONOTONE, thresh=THRESH)
    assert np.array_equal(fit.lambda_, NONMONOTONE) and (fit.return_codes == 0).all()
    assert_optimal(sa.kkt(fit, x, y), fit.lambda_, ("user lambdas", sparse))
    # every lambda's optimum is its own: the same values in decreasing order give the same coefficients
    order = np.argsort(NONMONOTONE)[::-1]
    mono = sa.sgdnet_newton(x, y, alpha=0.5, lambda_=np.array(NONMONOTONE)[order], thresh=THRESH)
    assert np.abs(fit.beta[:, order] - mono.beta).max() <= 1e-9 * np.abs(mono.beta).max()
    assert np.abs(fit.a0[order] - mono.a0).max() <= 1e-9 * max(1.0, np.abs(mono.a0).max())


def test_max_iter_is_reported(sa):
    x, y = problem(65, 16, False, seed=2)
    fit = sa.sgdnet_newton(x, y, alpha=0.5, nlambda=5, lambda_min_ratio=1e-2, thresh=1e-14, maxit=1)
    # one Newton step per lambda: one state pass at the start and one per step, more only where a step was halved
    assert (fit.return_codes[1:] == 1).all() and fit.npasses >= 1 + 5


# ---- (ii) the same problem and the same optimum as the existing solvers ----

def test_same_lambdas_and_nulldev_as_exact_mode(sa):
    x, y = abalone_binomial()
    for kw in (ABALONE, dict(ABALONE, intercept=False), dict(ABALONE, standardize=False, alpha=1.0)):
        newton = sa.sgdnet_newton(x, y, **kw)
        exact = sa.sgdnet(x, y, family="binomial", mode="exact", **kw)
        assert newton.lambda_.tobytes() == exact.lambda_.tobytes()
        assert newton.nulldev == exact.nulldev
    xs, ys = problem(300, 6, True, seed=9)
    newton = sa.sgdnet_newton(xs, ys, nlambda=5)
    exact = sa.sgdnet(xs, ys, family="binomial", nlambda=5, mode="exact")
    assert newton.lambda_.tobytes() == exact.lambda_.tobytes() and newton.nulldev == exact.nulldev


def test_same_optimum_as_the_oracle_on_abalone(sa, oracle):
    x, y = abalone_binomial()
    ref = oracle.fit(x, y, family="binomial", thresh=ORACLE_THRESH, maxit=100000, seed=1, **ABALONE)
    fit = sa.sgdnet_newton(x, y, thresh=THRESH, **ABALONE)
    assert (fit.return_codes == 0).all()
    assert np.allclose(fit.lambda_, ref["lambda"], rtol=1e-12)
    scale = np.abs(ref["beta"]).max()
    err = np.abs(fit.beta - ref["beta"][0]).max() / scale
    print("abalone: newton vs oracle, max coefficient difference / max|beta| = %.3g" % err)
    assert err <= ORACLE_TOL
    # intercepts and deviances below lambda_max only: there the oracle's stopping rule (coefficients only, all zero) leaves
    # ITS intercept short of its optimum
    assert np.abs(fit.a0[1:] - ref["a0"][0, 1:]).max() <= ORACLE_TOL * max(1.0, np.abs(ref["a0"]).max())
    assert np.abs(fit.dev_ratio[1:] - ref["dev_ratio"][1:]).max() <= ORACLE_TOL
    assert_optimal(sa.kkt(fit, x, y), fit.lambda_, "abalone")


# ---- (iii) degenerate columns ----

def test_all_zero_sparse_column(sa):
    x, y = problem(120, 6, True, seed=3)
    x = sp.csc_matrix(sp.hstack([x[:, :2], sp.csc_matrix((120, 1)), x[:, 3:]]))
    for mix in (0.0, 1.0):
        fit = sa.sgdnet_newton(x, y, alpha=mix, nlambda=8, lambda_min_ratio=1e-2, thresh=THRESH)
        assert (fit.beta[2] == 0.0).all() and (fit.return_codes == 0).all() and np.isfinite(fit.beta).all()
        assert_optimal(sa.kkt(fit, x, y), fit.lambda_, ("zero column", mix))


def test_constant_dense_column(sa):
    x, y = problem(120, 6, False, seed=4)
    x[:, 4] = 3.0
    for mix in (0.0, 1.0):
        for standardize in (True, False):
            fit = sa.sgdnet_newton(x, y, alpha=mix, nlambda=8, lambda_min_ratio=1e-2, thresh=THRESH, standardize=standardize)
            assert (fit.beta[4] == 0.0).all() and (fit.return_codes == 0).all() and np.isfinite(fit.beta).all()
            assert_optimal(sa.kkt(fit, x, y, standardize=standardize), fit.lambda_, ("constant column", mix, standardize))


def test_two_identical_columns_lasso(sa):
    x, y = problem(120, 6, False, seed=5)
    x[:, 5] = x[:, 1]
    fit = sa.sgdnet_newton(x, y, alpha=1.0, nlambda=8, lambda_min_ratio=1e-2, thresh=THRESH)
    assert (fit.return_codes == 0).all() and np.isfinite(fit.beta).all() and np.isfinite(fit.a0).all()
    assert_optimal(sa.kkt(fit, x, y), fit.lambda_, "identical columns")


# ---- (iv) cancellation: |mean| >> sd ----

@pytest.mark.parametrize("sparse", [False, True])
def test_large_mean_column_does_not_cancel(sa, sparse):
    x, _ = problem(200, 5, sparse, seed=7)
    rng = np.random.default_rng(11)
    col = rng.standard_normal(200)
    col = (col - col.mean()) / col.std()                      # sd 1; the column below has mean 1e6 (every entry stored)
    xd = np.asarray(x.todense()) if sparse else x.copy()
    shifted, centred = xd.copy(), xd.copy()
    shifted[:, 2], centred[:, 2] = 1e6 + col, col
    eta = 0.4 * (centred[:, 0] - centred[:, 0].mean()) + 1.2 * col
    y = (rng.random(200) < 1.0 / (1.0 + np.exp(-eta))).astype(float)
    kw = dict(alpha=0.5, nlambda=10, lambda_min_ratio=0.05, thresh=THRESH)
    wrap = sp.csc_matrix if sparse else np.asarray
    a, b = sa.sgdnet_newton(wrap(shifted), y, **kw), sa.sgdnet_newton(wrap(centred), y, **kw)
    assert (a.return_codes == 0).all() and (b.return_codes == 0).all()
    assert_optimal(sa.kkt(b, wrap(centred), y), b.lambda_, ("centred twin", sparse))
    scale = np.abs(b.beta).max()
    print("mean 1e6 vs centred: max coefficient difference / max|beta| = %.3g" % (np.abs(a.beta - b.beta).max() / scale))
    assert np.abs(a.lambda_ - b.lambda_).max() <= ORACLE_TOL * b.lambda_.max()
    assert np.abs(a.beta - b.beta).max() <= ORACLE_TOL * scale
    assert np.abs(a.dev_ratio - b.dev_ratio).max() <= ORACLE_TOL


# ---- (v) determinism and the generator ----

@pytest.mark.parametrize("sparse", [False, True])
def test_bitwise_repeatable_and_draws_nothing(sa, sparse):
    from sgdnet_amd import _lib, api
    x, y = problem(1003, 33, sparse, seed=8)
    kw = dict(alpha=0.5, nlambda=10, lambda_min_ratio=1e-2, thresh=1e-9)
    a = sa.sgdnet_newton(x, y, **kw)
    b = sa.sgdnet_newton(x, y, **kw)
    assert a.beta.tobytes() == b.beta.tobytes() and a.a0.tobytes() == b.a0.tobytes()
    assert a.dev_ratio.tobytes() == b.dev_ratio.tobytes()
    assert a.draws_used == 0 and b.draws_used == 0 and a.npasses == b.npasses > 0
    # a generator handed to the backend (what the R shim does with .Random.seed) comes back as it went
    rng = sa.RRng(3)
    before = bytes(rng.state)
    c = newton_with(api, _lib, x, y, rng=rng, **kw)
    assert bytes(rng.state) == before and c.beta.tobytes() == a.beta.tobytes() and c.draws_used == 0


def newton_with(api, _lib, x, y, family="binomial", alpha=1, nlambda=100, lambda_min_ratio=None, thresh=1e-3, **over):
    """sgdnet_newton's call of the shared front end with arguments sgdnet_newton itself does not pass on."""
    kw = dict(debug=False, seed=0, rng=None, sample_stream=None, unif=None, mode="newton", modes={"newton": _lib.MODE_NEWTON}, batch=0,
              device=0, devices=None)
    kw.update(over)
    return api._fit(x, y, family, alpha, nlambda, lambda_min_ratio, None, 1000, True, True, thresh, False, **kw)


# ---- (vi) refusals ----

def test_refusals_name_the_condition(sa):
    from sgdnet_amd import _lib, api

    def refused(needle, x, y, **kw):
        with pytest.raises(sa.SgdnetError) as e:
            newton_with(api, _lib, x, y, nlambda=3, **kw)
        assert e.value.code == -5, str(e.value)                   # SGDNET_EUNSUPPORTED
        assert "mode = newton needs" in str(e.value) and needle in str(e.value), str(e.value)

    rng = np.random.default_rng(0)
    x = rng.standard_normal((60, 4))
    y = x[:, 0] + rng.standard_normal(60)
    cls = (y > 0).astype(float)
    wide = rng.standard_normal((20, pmax() + 1))
    wide_cls = (wide[:, 0] > 0).astype(float)
    refused("features (limit %d)" % pmax(), wide, wide_cls)
    refused("sgdnet_newton_max_features", sp.csc_matrix(wide), wide_cls)
    with pytest.raises(sa.SgdnetError, match="mode = newton needs no more features"):
        sa.sgdnet_newton(wide, wide_cls, nlambda=3)
    refused("family = binomial", x, y, family="gaussian")
    refused("family = binomial", x, np.digitize(y, [-0.5, 0.5]), family="multinomial")
    refused("family = binomial", x, np.column_stack([y, -y]), family="mgaussian")
    refused("one GPU", x, cls, devices=[0, 0])
    refused("one GPU", sp.csc_matrix(x), cls, devices=[0, 0])
    refused("debug = 0", x, cls, debug=True)
    # sgdnet() does not know the mode, and no mode of sgdnet() reaches the Newton loop: the SAGA modes still draw
    with pytest.raises(ValueError, match="mode must be one of 'exact', 'batched', 'auto', 'covariance'$"):
        sa.sgdnet(x, cls, family="binomial", nlambda=3, mode="newton")
    assert sa.sgdnet(x, cls, family="binomial", nlambda=3, mode="auto").draws_used > 0


# ---- (vii) the R shim ----

@pytest.mark.parametrize("sparse", [False, True])
def test_shim_option_gives_the_ctypes_fit(sa, sparse):
    import rshim
    R = rshim.lib()
    R.rmock_reset()
    R.R_init_sgdnet(None)
    n, p, nl = 300, 6, 12
    x, y = problem(n, p, sparse, seed=9)
    rshim.set_option("sgdnet.mode", "newton")
    R.rmock_set_seed(7)
    ctl = rshim.control_list(family="binomial", alpha=0.5, nlambda=nl, lambda_min_ratio=1e-3, thresh=1e-9, maxit=1000, is_sparse=sparse)
    got = rshim.decode_result(rshim.call("_sgdnet_SgdnetSparse" if sparse else "_sgdnet_SgdnetDense",
                                         rshim.r_dgcmatrix(x) if sparse else rshim.r_matrix(x), rshim.r_matrix(y.reshape(n, 1)), ctl))
    ref = sa.sgdnet_newton(x, y, alpha=0.5, nlambda=nl, lambda_min_ratio=1e-3, thresh=1e-9, maxit=1000)
    assert got["unlist_beta"].tobytes() == ref.beta.ravel(order="F").tobytes()
    assert got["a0"][0].tobytes() == ref.a0.tobytes() and got["lambda_"].tobytes() == ref.lambda_.tobytes()
    assert got["dev_ratio"].tobytes() == ref.dev_ratio.tobytes() and got["npasses"] == ref.npasses
    assert R.rmock_unif_count() == 0 and R.rmock_protect_depth() == 0
