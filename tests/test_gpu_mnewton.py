"""sa.sgdnet_mnewton (SGDNET_MODE_MNEWTON, sgdnet_amd/csrc/mnewton.hip): the multinomial elastic-net path solved to its
optimum by proximal Newton steps on the joint Hessian of all K (p + 1) coordinates.  Checked against the optimality
conditions of the problem the driver solves (sa.kkt: device gradient on the data as it came + the numpy conventions of
sgdnet_amd/kkt.py); the shapes sit at the kernels' edges (the 16-column tiles of the moments pass with p + 2 columns one
below, at and above an edge; the 64-row staging step and the first second row chunk at 257 rows; one stride of the inner
solve's wavefront; one workgroup's LDS at p = mnewton_max_features(K)).

At mix = 1 and an even K the optimum need not be unique in the coefficients (adding the same vector to the coefficients
of every class changes no eta; the l1 norm is flat along it between two medians): there only the certificate and the
deviance are compared, never coefficients.

numpy_mnewton_path() and numpy_kkt() below restate the algorithm and the certificate in numpy;
tests/test_mnewton_host.py checks on the CPU that the restatement's optimum stays inside the bound used here for the
same inputs, and measures the oracle's distance from its own optimum (ORACLE_* below).

Seen on an MI355X (the optimality tests): worst KKT ratio 9.25e-10 (iris, mix 1, no intercept, no standardisation) and
worst intercept residual 1.65e-11 lambda -- the restatement's own figures on the same inputs -- dev_ratio within 7.5e-15
of the returned coefficients'."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp

import test_gpu_covariance as tc

pytestmark = pytest.mark.gpu
GOLD = tc.GOLD

# The project's optimality bound (tests/test_gpu_newton.py): KKT residual <= 1e-8 * lambda, for the coefficients and for
# the intercepts (class mean removed).
KKT_BOUND = tc.KKT_BOUND
THRESH = 1e-12                                   # test_gpu_newton.py's
SETTINGS = [(True, True), (True, False), (False, True), (False, False)]                # (intercept, standardize)
MIXES = [1.0, 0.5, 0.0]
NLAMBDA = 5


def kernel_constants():
    """(tile columns, rows staged per step, rows per row chunk below which one chunk does) from csrc/moments_device.hpp:
    kTileCols, kTileRows and the divisor of dense_rows_per_chunk's chunk count."""
    src = open(os.path.join(os.path.dirname(GOLD), os.pardir, "sgdnet_amd", "csrc", "moments_device.hpp")).read()
    cols = int(re.search(r"constexpr int kTileCols = (\d+);", src).group(1))
    rows = int(re.search(r"constexpr int kTileRows = (\d+);", src).group(1))
    m = re.search(r"const int64_t chunks = std::min<int64_t>\(chunk_cap, \(n \+ (\d+)\) / (\d+)\);", src)
    assert int(m.group(1)) + 1 == int(m.group(2))
    return cols, rows, int(m.group(2))


TILE_COLS, TILE_ROWS, CHUNK_ROWS = kernel_constants()
# (n, p, K); p = None: sa.mnewton_max_features(K).  Tile edges: p + 2 columns one below, at and above a tile edge.  Rows:
# one below, at and above the staging step and the row count at which the moments pass opens its second row chunk.
TILE_SHAPES = [(90, TILE_COLS - 3, 3), (90, TILE_COLS - 2, 3), (90, TILE_COLS - 1, 3)]
ROW_SHAPES = [(n, 3, 3) for n in (TILE_ROWS - 1, TILE_ROWS, TILE_ROWS + 1, CHUNK_ROWS - 1, CHUNK_ROWS, CHUNK_ROWS + 1)]
CLASS_SHAPES = [(120, 5, 2), (160, 5, 4), (200, 6, 5)]
LIMIT_SHAPES = [(300, None, 2), (300, None, 3)]
NONMONOTONE = [0.03, 0.004, 0.08, 0.01]
# the constants of csrc/newton.hpp, restated for numpy_mnewton_path
MAX_HALVINGS, OBJECTIVE_SLACK, MAX_SWEEPS, NEGLIGIBLE = 10, 1e-12, 1000, 16 * 2.220446049250313e-16

# The CPU oracle (SAGA) on iris at mix = 0.5 and 0, where the optimum is unique.  Per mix: the distance of the oracle at
# ORACLE_THRESH from the numpy restatement's optimum -- coefficients relative to max|beta|, class-centred intercepts
# relative to max(1, max|a0|), dev_ratio absolute -- measured and pinned by
# test_mnewton_host.py::test_oracle_distance_from_the_optimum_on_iris; the tolerances are 10 x these, the margin
# test_gpu_mcovariance.py gives its ORACLE_* constants.
ORACLE_THRESH = 1e-9
ORACLE_PATH = dict(nlambda=8, lambda_min_ratio=1e-2)
ORACLE_MIXES = [0.5, 0.0]
ORACLE_BETA_DIST = {0.5: 8.0e-9, 0.0: 8.7e-10}     # measured 7.95e-9, 8.59e-10
ORACLE_A0_DIST = {0.5: 5.2e-9, 0.0: 3.0e-8}        # measured 5.12e-9, 2.95e-8
ORACLE_DEV_DIST = {0.5: 1.4e-10, 0.0: 5.7e-11}     # measured 1.36e-10, 5.62e-11


def pmax(K):
    import sgdnet_amd as sa
    return sa.mnewton_max_features(K)


def iris():
    d = np.load(os.path.join(GOLD, "iris.npz"))
    return np.asarray(d["x"], dtype=float), np.asarray(d["y"], dtype=float)


def problem(n, p, K, sparse=False, seed=0):
    """x as test_gpu_covariance.problem makes it (columns of different means and scales; sparse: part of the entries
    stored); class codes 0 .. K - 1 drawn from the softmax model with coefficients B / sqrt(p / 4) on the centred
    columns, half of B's rows zero, every class at least twice."""
    x, _ = tc.problem(n, p, sparse, seed)
    xd = np.asarray(x.todense()) if sparse else x
    rng = np.random.default_rng(7000 * seed + 13 * n + 5 * p + K)
    B = rng.standard_normal((p, K)) * (rng.random(p) < 0.5)[:, None] / np.sqrt(p / 4)
    eta = (xd - xd.mean(axis=0)) @ B + rng.uniform(-0.5, 0.5, K)
    pr = np.exp(eta - eta.max(axis=1, keepdims=True))
    pr /= pr.sum(axis=1, keepdims=True)
    y = (pr.cumsum(axis=1) < rng.random(n)[:, None]).sum(axis=1).clip(0, K - 1).astype(float)
    y[:2 * K] = np.repeat(np.arange(K), 2)                       # every class at least twice
    return x, y


def dense(x):
    return np.asarray(x.todense()) if sp.issparse(x) else np.asarray(x, dtype=float)


def null_intercepts(y, K, intercept):
    """fit_null_model of the driver for multinomial: the centred logs of the class proportions (1 / K without an intercept)."""
    pr = np.bincount(y.astype(int), minlength=K) / len(y) if intercept else np.full(K, 1.0 / K)
    return np.log(pr) - np.log(pr).mean()


def automatic_lambdas(x, y, K, mix, standardize, nlambda, ratio):
    """regularization_path / lambda_max of the driver for a multinomial response (driver.cpp)."""
    import sgdnet_amd as sa
    xd = dense(x)
    xc, xs = sa.feature_moments(x, standardize)
    Y = np.eye(K)[y.astype(int)]
    lmax = np.abs(((xd - xc) / xs).T @ (Y - Y.mean(axis=0))).max() / len(y) / max(mix, 0.001)
    return np.exp(np.linspace(np.log(lmax), np.log(lmax * ratio), nlambda))


def numpy_mnewton_path(x, y, K, lam, mix, standardize=True, intercept=True, thresh=THRESH, maxit=1000):
    """The algorithm of csrc/mnewton.hip in numpy, in the driver's units (sgdnet_amd/kkt.py): per outer step the state
    (mu, loss) at the iterate, the joint Hessian and gradient of all K (p + 1) coordinates over [x - m | 1] / s, cyclic
    coordinate descent on the penalised quadratic model (the intercepts unpenalised; never visited without an
    intercept), halving while the objective rose.  Returns (a0 (K, L), beta (K, p, L), dev_ratio (L), info)."""
    x = dense(x)
    n, p = x.shape
    P, Q = p + 1, K * (p + 1)
    mean = x.mean(axis=0)
    var = ((x - mean) ** 2).mean(axis=0)
    sd = np.where(var == 0, 1.0, np.sqrt(var)) if standardize else np.ones(p)
    m = mean if (standardize or intercept) else np.zeros(p)
    Z = np.column_stack([(x - m) / sd, np.ones(n)])
    yi = y.astype(int)
    Y = np.eye(K)[yi]
    b0 = null_intercepts(y, K, intercept)
    u = np.zeros((K, P))
    u[:, p] = b0
    u = u.ravel()
    pen = np.tile(np.arange(P) < p, K)                            # penalised coordinates
    visit = [j for j in range(Q) if pen[j] or intercept]

    def state(u):
        eta = Z @ u.reshape(K, P).T
        mx = eta.max(axis=1, keepdims=True)
        e = np.exp(eta - mx)
        s = e.sum(axis=1, keepdims=True)
        return e / s, (np.log(s[:, 0]) + mx[:, 0] - eta[np.arange(n), yi]).mean()

    def penalty(u, l1, l2):
        return l2 * 0.5 * (u[pen] ** 2).sum() + l1 * np.abs(u[pen]).sum()

    pr0 = np.bincount(yi, minlength=K) / n if intercept else np.full(K, 1.0 / K)
    nulldev = -2.0 * np.log(pr0[yi]).sum()
    mu, loss = state(u)
    info = dict(halvings=0, steps=[], codes=[], passes=1, sweeps=0)
    a0, beta, dev = [], [], []
    for l in lam:
        l1, l2 = (0.0 if mix == 0 else mix * l), (1 - mix) * l
        objective = loss + penalty(u, l1, l2)
        steps, converged = 0, False
        while steps < maxit and not converged:
            H = np.empty((Q, Q))
            for k in range(K):
                for kk in range(k, K):
                    wgt = mu[:, k] * ((1.0 if k == kk else 0.0) - mu[:, kk])
                    blk = (Z * wgt[:, None]).T @ Z / n
                    H[k * P:(k + 1) * P, kk * P:(kk + 1) * P] = blk
                    H[kk * P:(kk + 1) * P, k * P:(k + 1) * P] = blk
            q = (Z.T @ (Y - mu) / n).T.ravel()
            c, g = u.copy(), -q
            diag = np.diag(H).copy()
            inner = negligible = False
            for _ in range(MAX_SWEEPS):
                change = size = eta_sq = 0.0
                for j in visit:
                    hjj = diag[j]
                    z, den = hjj * c[j] - g[j], hjj + (l2 if pen[j] else 0.0)
                    nu = z
                    if pen[j] and mix != 0:
                        nu = z - l1 if z > l1 else (z + l1 if z < -l1 else 0.0)
                    nu = nu / den if den > 0 else c[j]
                    if pen[j] and mix != 0 and nu * nu * hjj <= NEGLIGIBLE ** 2:      # the threshold's rounding residue: exactly 0
                        nu = 0.0
                    d = nu - c[j]
                    change, size, eta_sq = max(change, abs(d)), max(size, abs(nu)), max(eta_sq, nu * nu * hjj)
                    if d != 0.0:
                        c[j] = nu
                        g += H[:, j] * d
                info["sweeps"] += 1
                negligible = eta_sq <= NEGLIGIBLE ** 2                  # zero to rounding (newton.hpp)
                if (size == 0 and change == 0) or (size != 0 and change / size <= thresh) or negligible:
                    inner = True
                    break
            mu, cl = state(c)
            info["passes"] += 1
            candidate = cl + penalty(c, l1, l2)
            h = 0
            while h < MAX_HALVINGS and np.abs(c - u).max() > 0 and not candidate <= objective + OBJECTIVE_SLACK * abs(objective):
                c = u + 0.5 * (c - u)
                mu, cl = state(c)
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
        U = u.reshape(K, P)
        b = U[:, :p] / sd
        icpt = U[:, p] - b @ m if intercept else b0.copy()
        a0.append(icpt - icpt.mean() if intercept else icpt)
        beta.append(b)
        dev.append(1.0 - 2.0 * n * loss / nulldev)
    return np.array(a0).T, np.moveaxis(np.array(beta), 0, 2), np.array(dev), info


def as_fit(a0, beta, lam, mix):
    return SimpleNamespace(a0=np.asarray(a0), beta=np.asarray(beta), lambda_=np.asarray(lam, dtype=float), alpha=mix, family="multinomial")


def stacked(fit):
    return np.stack([np.asarray(b) for b in fit.beta])              # (K, p, L)


def numpy_probabilities(a0, beta, x, y, standardize, intercept):
    """(mu (n, K, L), Y (n, K)) at the predictor the driver made stationary (kkt.py: evaluation_intercepts)."""
    import sgdnet_amd as sa
    beta = np.asarray(beta)
    xc, _ = sa.feature_moments(x, standardize)
    ev = sa.evaluation_intercepts(SimpleNamespace(a0=np.asarray(a0), beta=beta), xc, None, intercept)     # (K, L)
    eta = ev[None] + np.einsum("ij,kjl->ikl", dense(x), beta)
    e = np.exp(eta - eta.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True), np.eye(beta.shape[0])[np.asarray(y).astype(int)]


def numpy_kkt(a0, beta, x, y, lam, mix, standardize, intercept):
    """sa.kkt without the device: the gradient of the multinomial loss in numpy, then kkt_from_gradient."""
    import sgdnet_amd as sa
    fit = as_fit(a0, beta, lam, mix)
    xc, xs = sa.feature_moments(x, standardize)
    mu, Y = numpy_probabilities(a0, beta, x, y, standardize, intercept)
    r = mu - Y[:, :, None]                                                          # families.h Gradient
    G, G0 = np.einsum("ij,ikl->kjl", dense(x), r) / len(Y), r.mean(axis=0)
    return sa.kkt_from_gradient(G, G0, fit, x_center=xc, x_scale=xs, y_scale=None, standardize=standardize, intercept=intercept)


def numpy_dev_ratio(a0, beta, x, y, standardize, intercept):
    """1 - deviance / null deviance from the returned coefficients, as the driver defines both for multinomial."""
    mu, Y = numpy_probabilities(a0, beta, x, y, standardize, intercept)
    K = Y.shape[1]
    pr0 = Y.mean(axis=0) if intercept else np.full(K, 1.0 / K)
    nulldev = -2.0 * (Y * np.log(pr0)).sum()
    return 1.0 - (-2.0 * np.log((mu * Y[:, :, None]).sum(axis=1)).sum(axis=0)) / nulldev


# dev_ratio against the deviance of the returned coefficients: n terms of size <= log K + |eta| each rounded to 1e-16
# relative, and a coefficient within KKT_BOUND lambda of stationarity moves the deviance at second order only
DEV_TOL = 1e-10


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


def check_fit(sa, fit, x, y, what, standardize=True, intercept=True):
    assert fit.family == "multinomial" and (fit.return_codes == 0).all() and fit.draws_used == 0 and np.isfinite(fit.dev_ratio).all(), what
    k = sa.kkt(fit, x, y, standardize=standardize, intercept=intercept)
    assert_optimal(k, fit.lambda_, what)
    ref = numpy_dev_ratio(fit.a0, stacked(fit), x, y, standardize, intercept)
    print(what, "dev_ratio vs numpy max %.3g" % np.abs(fit.dev_ratio - ref).max())
    assert np.abs(fit.dev_ratio - ref).max() <= DEV_TOL, what
    if intercept:                                                   # the documented convention: class mean removed
        assert np.abs(np.asarray(fit.a0).mean(axis=0)).max() <= 1e-12 * max(1.0, np.abs(fit.a0).max())


def ratio_for(shape):
    return 5e-2 if shape[1] is None else 1e-2


def fit_all_settings(sa, x, y, shape, mix, nlambda=NLAMBDA):
    n, p, K = shape[0], shape[1] or pmax(shape[2]), shape[2]
    for intercept, standardize in SETTINGS:
        fit = sa.sgdnet_mnewton(x, y, alpha=mix, nlambda=nlambda, lambda_min_ratio=ratio_for(shape), thresh=THRESH, intercept=intercept,
                                standardize=standardize)
        assert len(fit.beta) == K and fit.beta[0].shape == (p, nlambda)
        check_fit(sa, fit, x, y, (n, p, K, mix, intercept, standardize), standardize, intercept)


# ---- (i) optimality and deviance across the envelope ----

@pytest.mark.parametrize("mix", MIXES)
def test_iris_path_is_optimal(sa, mix):
    x, y = iris()
    fit_all_settings(sa, x, y, (150, 4, 3), mix, nlambda=6)


@pytest.mark.parametrize("mix", MIXES)
@pytest.mark.parametrize("shape", TILE_SHAPES + ROW_SHAPES + CLASS_SHAPES)
def test_automatic_path_is_optimal(sa, shape, mix):
    x, y = problem(*shape)
    fit_all_settings(sa, x, y, shape, mix)


@pytest.mark.parametrize("mix", MIXES)
@pytest.mark.parametrize("shape", LIMIT_SHAPES)
def test_path_at_the_feature_limit_is_optimal(sa, shape, mix):
    n, K = shape[0], shape[2]
    x, y = problem(n, pmax(K), K)
    fit_all_settings(sa, x, y, shape, mix, nlambda=4)


def test_user_lambdas_need_not_be_monotone(sa):
    x, y = problem(200, 6, 5, seed=2)
    fit = sa.sgdnet_mnewton(x, y, alpha=0.5, lambda_=NONMONOTONE, thresh=THRESH)
    assert np.array_equal(fit.lambda_, NONMONOTONE)
    check_fit(sa, fit, x, y, "user lambdas")
    # every lambda's optimum is its own (unique at mix 0.5): the same values in decreasing order give the same coefficients
    order = np.argsort(NONMONOTONE)[::-1]
    mono = sa.sgdnet_mnewton(x, y, alpha=0.5, lambda_=np.array(NONMONOTONE)[order], thresh=THRESH)
    assert np.abs(stacked(fit)[:, :, order] - stacked(mono)).max() <= 1e-9 * np.abs(stacked(mono)).max()


def test_max_iter_is_reported(sa):
    x, y = problem(200, 6, 5, seed=3)
    fit = sa.sgdnet_mnewton(x, y, alpha=0.5, nlambda=5, lambda_min_ratio=1e-2, thresh=1e-14, maxit=1)
    assert (fit.return_codes[1:] == 1).all() and np.isfinite(stacked(fit)).all() and np.isfinite(fit.dev_ratio).all()
    assert 1 + 4 <= fit.npasses <= 1 + 5 * (1 + MAX_HALVINGS)


def test_lambda_max_first(sa):
    """The automatic path starts at lambda_max: all coefficients exactly zero there, the intercepts at the null model."""
    x, y = iris()
    for intercept, standardize in SETTINGS:
        for mix in (1.0, 0.5):
            fit = sa.sgdnet_mnewton(x, y, alpha=mix, nlambda=4, thresh=THRESH, intercept=intercept, standardize=standardize)
            assert (stacked(fit)[:, :, 0] == 0.0).all(), (intercept, standardize, mix, stacked(fit)[:, :, 0])
            assert np.abs(np.asarray(fit.a0)[:, 0] - null_intercepts(y, 3, intercept)).max() <= 1e-12
            assert abs(fit.dev_ratio[0]) <= 1e-12 and fit.return_codes[0] == 0
    x, y = problem(200, 6, 5)                                       # classes of different sizes: intercepts away from 0
    fit = sa.sgdnet_mnewton(x, y, alpha=1.0, nlambda=4, thresh=THRESH)
    assert (stacked(fit)[:, :, 0] == 0.0).all()
    assert np.abs(np.asarray(fit.a0)[:, 0] - null_intercepts(y, 5, True)).max() <= 1e-12


# ---- (ii) sparse x: the same dense path ----

@pytest.mark.parametrize("mix", MIXES)
@pytest.mark.parametrize("shape", [(150, 4, 3)] + TILE_SHAPES + ROW_SHAPES + CLASS_SHAPES + LIMIT_SHAPES)
def test_sparse_x_gives_the_bits_of_its_dense_copy(sa, shape, mix):
    """The driver expands sparse x before anything is computed from it: the automatic path, the standard deviations and
    the fit are those of x.toarray(), bit for bit, in every setting."""
    n, K = shape[0], shape[2]
    p = shape[1] or pmax(K)
    xs, y = problem(n, p, K, sparse=True)
    assert sp.issparse(xs)
    for intercept, standardize in SETTINGS:
        kw = dict(alpha=mix, nlambda=4, lambda_min_ratio=ratio_for(shape), thresh=THRESH, intercept=intercept, standardize=standardize)
        a, b = sa.sgdnet_mnewton(xs, y, **kw), sa.sgdnet_mnewton(xs.toarray(), y, **kw)
        assert a.lambda_.tobytes() == b.lambda_.tobytes() and a.nulldev == b.nulldev
        assert stacked(a).tobytes() == stacked(b).tobytes() and np.asarray(a.a0).tobytes() == np.asarray(b.a0).tobytes()
        assert a.dev_ratio.tobytes() == b.dev_ratio.tobytes() and a.npasses == b.npasses
        assert (a.return_codes == 0).all() and a.draws_used == 0
    check_fit(sa, a, xs, y, ("sparse", shape, mix), standardize, intercept)


def test_sparse_entries_stored_twice_add_up(sa):
    xs, y = problem(160, 5, 4, sparse=True)
    c = xs.tocoo()
    twice = sp.csc_matrix((np.concatenate([0.25 * c.data, 0.75 * c.data]), (np.tile(c.row, 2), np.tile(c.col, 2))), shape=xs.shape)
    twice_raw = sp.csc_matrix(xs.shape)
    twice_raw.indptr, twice_raw.indices, twice_raw.data = twice.indptr, twice.indices, twice.data
    kw = dict(alpha=0.5, nlambda=4, lambda_min_ratio=1e-2, thresh=THRESH)
    a, b = sa.sgdnet_mnewton(twice, y, **kw), sa.sgdnet_mnewton(xs, y, **kw)
    assert np.abs(stacked(a) - stacked(b)).max() <= 1e-9 * np.abs(stacked(b)).max()


# ---- (iii) the same lambdas as, and the same optimum as, the existing solvers ----

def test_same_lambdas_and_null_deviance_as_exact_mode(sa):
    x, y = iris()
    kw = dict(alpha=0.5, nlambda=12, lambda_min_ratio=1e-2)
    new = sa.sgdnet_mnewton(x, y, **kw)
    exact = sa.sgdnet(x, y, family="multinomial", mode="exact", **kw)
    assert new.lambda_.tobytes() == exact.lambda_.tobytes() and new.nulldev == exact.nulldev


def centred(a0):
    a0 = np.asarray(a0)
    return a0 - a0.mean(axis=0, keepdims=True)


@pytest.mark.parametrize("mix", ORACLE_MIXES)
def test_same_optimum_as_the_oracle_on_iris(sa, oracle, mix):
    x, y = iris()
    ref = oracle.fit(x, y, family="multinomial", n_classes=3, alpha=mix, thresh=ORACLE_THRESH, maxit=100000, seed=1, **ORACLE_PATH)
    fit = sa.sgdnet_mnewton(x, y, alpha=mix, thresh=THRESH, **ORACLE_PATH)
    assert (fit.return_codes == 0).all() and (ref["return_codes"] == 0).all()
    assert np.allclose(fit.lambda_, ref["lambda"], rtol=1e-12, atol=0)
    rb, ra = np.asarray(ref["beta"]).reshape(stacked(fit).shape), centred(np.asarray(ref["a0"]).reshape(np.asarray(fit.a0).shape))
    err = np.abs(stacked(fit) - rb).max() / np.abs(rb).max()
    a0_err = np.abs(centred(fit.a0)[:, 1:] - ra[:, 1:]).max() / max(1.0, np.abs(ra).max())
    dev_err = np.abs(fit.dev_ratio[1:] - ref["dev_ratio"][1:]).max()
    print("mix %g vs oracle: coefficients %.3g (tol %.3g) intercepts %.3g (tol %.3g) dev_ratio %.3g (tol %.3g)"
          % (mix, err, 10 * ORACLE_BETA_DIST[mix], a0_err, 10 * ORACLE_A0_DIST[mix], dev_err, 10 * ORACLE_DEV_DIST[mix]))
    assert err <= 10 * ORACLE_BETA_DIST[mix]
    assert a0_err <= 10 * ORACLE_A0_DIST[mix]
    assert dev_err <= 10 * ORACLE_DEV_DIST[mix]


# ---- (iv) degenerate inputs ----

def test_constant_column(sa):
    x, y = problem(160, 5, 4, seed=5)
    x[:, 2] = 3.0
    for mix in MIXES:
        for standardize in (True, False):
            fit = sa.sgdnet_mnewton(x, y, alpha=mix, nlambda=5, lambda_min_ratio=1e-2, thresh=THRESH, standardize=standardize)
            assert (stacked(fit)[:, 2] == 0.0).all() and np.isfinite(stacked(fit)).all()
            check_fit(sa, fit, x, y, ("constant column", mix, standardize), standardize=standardize)


def test_class_with_a_single_member(sa):
    """sgdnet()'s validation refuses such a response; the backend takes it (the R front end's check is not the shim's)."""
    from sgdnet_amd import _lib, api
    x, y = problem(120, 4, 3, seed=6)
    y[y == 2] = 1.0
    y[7] = 2.0
    assert (y == 2).sum() == 1
    with pytest.raises(ValueError, match="one class only has 1 observations"):
        sa.sgdnet_mnewton(x, y, nlambda=3)
    fit = native_fit(sa, x, y, 3, alpha=0.5, nlambda=5, lambda_min_ratio=1e-2, thresh=THRESH)
    check_fit(sa, fit, x, y, "single member")


def native_fit(sa, x, y, K, alpha, nlambda, lambda_min_ratio, thresh, maxit=1000):
    """SGDNET_MODE_MNEWTON through the native entry point on class codes, without sgdnet()'s checks of the response."""
    import ctypes as C
    from sgdnet_amd import _lib
    n, p = x.shape
    xf, ym = np.asfortranarray(x, dtype=np.float64), np.asfortranarray(y.reshape(-1, 1), dtype=np.float64)
    ctl = _lib.Control()
    ctl.elasticnet_mix, ctl.family, ctl.intercept, ctl.standardize = float(alpha), _lib.FAMILIES["multinomial"], 1, 1
    ctl.lambda_min_ratio, ctl.max_iter, ctl.n_lambda, ctl.n_classes, ctl.tol = lambda_min_ratio, maxit, nlambda, K, thresh
    ctl.mode = _lib.MODE_MNEWTON
    a0, beta = np.zeros((K, nlambda), order="F"), np.zeros((K, p, nlambda), order="F")
    lam, dev, codes = np.zeros(nlambda), np.zeros(nlambda), np.zeros(nlambda)
    res = _lib.Result()
    res.a0, res.beta, res.lambda_ = _lib.dptr(a0), _lib.dptr(beta), _lib.dptr(lam)
    res.dev_ratio, res.return_codes = _lib.dptr(dev), _lib.dptr(codes)
    _lib.check(_lib.load().sgdnet_fit_dense(_lib.dptr(xf), n, p, _lib.dptr(ym), 1, C.byref(ctl), C.byref(res)))
    return SimpleNamespace(a0=a0 - a0.mean(axis=0, keepdims=True), beta=[beta[k] for k in range(K)], lambda_=lam, dev_ratio=dev,
                           return_codes=codes, draws_used=res.draws_used, npasses=res.npasses, alpha=alpha, family="multinomial")


# ---- (v) determinism and the generator ----

@pytest.mark.parametrize("sparse", [False, True])
def test_bitwise_repeatable_and_draws_nothing(sa, sparse):
    x, y = problem(1003, 15, 4, sparse=sparse, seed=10)
    rng = sa.RRng(3)
    before = bytes(rng.state)
    kw = dict(alpha=0.5, nlambda=8, lambda_min_ratio=1e-2, thresh=1e-9)
    a = sa.sgdnet_mnewton(x, y, **kw)
    b = sa.sgdnet_mnewton(x, y, **kw)
    assert stacked(a).tobytes() == stacked(b).tobytes() and np.asarray(a.a0).tobytes() == np.asarray(b.a0).tobytes()
    assert a.dev_ratio.tobytes() == b.dev_ratio.tobytes()
    assert a.draws_used == 0 and b.draws_used == 0 and a.npasses == b.npasses > 0
    # a generator the caller holds is not advanced by the backend either
    c = mnewton_with(x, y, alpha=0.5, nlambda=8, lambda_min_ratio=1e-2, thresh=1e-9, rng=rng)
    assert bytes(rng.state) == before and stacked(c).tobytes() == stacked(a).tobytes()


# ---- (vi) refusals and dispatch ----

def mnewton_with(x, y, family="multinomial", alpha=0.5, nlambda=3, lambda_min_ratio=None, thresh=1e-3, lambda_=None, **over):
    from sgdnet_amd import _lib, api
    kw = dict(debug=False, seed=0, rng=None, sample_stream=None, unif=None, batch=0, device=0, devices=None)
    kw.update(over)
    return api._fit(x, y, family, alpha, nlambda, lambda_min_ratio, lambda_, 1000, True, True, thresh, False, mode="mnewton",
                    modes={"mnewton": _lib.MODE_MNEWTON}, min_classes=2, **kw)


def refused(sa, needle, x, y, **kw):
    with pytest.raises(sa.SgdnetError) as e:
        mnewton_with(x, y, **kw)
    assert e.value.code == -5, str(e.value)                   # SGDNET_EUNSUPPORTED
    assert "mode = mnewton needs " in str(e.value) and needle in str(e.value), str(e.value)


def test_refusals_name_the_condition(sa):
    rng = np.random.default_rng(0)
    x = rng.standard_normal((60, 4))
    y = np.arange(60) % 3
    refused(sa, "family = multinomial", x, (y > 0).astype(float), family="binomial")
    refused(sa, "family = multinomial", x, x[:, 0] + rng.standard_normal(60), family="gaussian")
    for K in (2, 3, 10):
        wide, yk = rng.standard_normal((40, pmax(K) + 1)), np.arange(40) % K
        refused(sa, "features (limit %d)" % pmax(K), wide, yk)
        refused(sa, "sgdnet_mnewton_max_features(n_classes)", sp.csc_matrix(wide), yk)
        assert mnewton_with(wide[:, :-1], yk, lambda_min_ratio=0.5).draws_used == 0                # the limit itself is taken
    refused(sa, "one GPU", x, y, devices=[0, 0])
    refused(sa, "debug = 0", x, y, debug=True)
    # the dense copy of a sparse x: n p 8 bytes > 1 GiB (a few stored entries; user lambdas keep the host passes short)
    n_big = (1 << 30) // (8 * 64) + 1
    big = sp.csc_matrix((np.ones(6), (np.arange(6), np.arange(6) % 64)), shape=(n_big, 64))
    refused(sa, "the dense copy of a sparse x", big, np.arange(n_big) % 3, lambda_=[0.1, 0.05], nlambda=2)


def test_the_other_doors_stay_shut(sa):
    x, y = iris()
    with pytest.raises(ValueError, match="mode must be one of"):
        sa.sgdnet(x, y, family="multinomial", nlambda=3, mode="mnewton")
    for mode, needle in (("covariance", "mode = covariance needs family = gaussian"),):
        with pytest.raises(sa.SgdnetError) as e:
            sa.sgdnet(x, y, family="multinomial", nlambda=3, mode=mode)
        assert e.value.code == -5 and needle in str(e.value)
    from sgdnet_amd import _lib, api
    for name, code, needle in (("newton", _lib.MODE_NEWTON, "mode = newton needs family = binomial"),
                               ("mcovariance", _lib.MODE_MCOVARIANCE, "mode = mcovariance needs family = mgaussian")):
        with pytest.raises(sa.SgdnetError) as e:
            api._fit(x, y, "multinomial", 0.5, 3, None, None, 1000, True, True, 1e-3, False, debug=False, seed=0, rng=None,
                     sample_stream=None, unif=None, mode=name, modes={name: code}, batch=0, device=0, devices=None)
        assert e.value.code == -5 and needle in str(e.value)
    # ... and auto does not reach the new mode: the SAGA modes still draw.  (The batched iteration of dense multi-class x
    # adds its workgroups' gradient sums with atomics, DESIGN.md 4.3: two auto fits of one input and seed differ in their last
    # bits, so "the same bits as an earlier build" is not defined for auto; that it draws is what shows the dispatch.)
    assert sa.sgdnet(x, y, family="multinomial", alpha=0.8, nlambda=5, mode="auto", seed=1).draws_used > 0
    assert sa.sgdnet_mnewton(x, y, alpha=0.8, nlambda=5).draws_used == 0


# ---- (vii) the R shim ----

@pytest.mark.parametrize("sparse", [False, True])
def test_shim_option_gives_the_ctypes_fit(sa, sparse):
    import rshim
    R = rshim.lib()
    R.rmock_reset()
    R.R_init_sgdnet(None)
    n, p, K, nl = 300, 6, 3, 8
    x, y = problem(n, p, K, sparse=sparse, seed=12)
    rshim.set_option("sgdnet.mode", "mnewton")
    R.rmock_set_seed(7)
    kw = dict(alpha=0.5, nlambda=nl, lambda_min_ratio=1e-3, thresh=1e-9, maxit=1000)
    ctl = rshim.control_list(family="multinomial", n_classes=K, is_sparse=sparse, **kw)
    got = rshim.decode_result(rshim.call("_sgdnet_SgdnetSparse" if sparse else "_sgdnet_SgdnetDense",
                                         rshim.r_dgcmatrix(x) if sparse else rshim.r_matrix(x), rshim.r_matrix(y.reshape(-1, 1)), ctl))
    ref = mnewton_with(x, y, **{k: v for k, v in kw.items() if k != "maxit"})
    assert got["unlist_beta"].tobytes() == stacked(ref).ravel(order="F").tobytes()
    # the shim returns the backend's intercepts (class mean removed there); sgdnet() removes the class mean once more
    assert np.abs(centred(got["a0"]) - np.asarray(ref.a0)).max() <= 1e-15 * max(1.0, np.abs(ref.a0).max())
    assert got["lambda_"].tobytes() == ref.lambda_.tobytes()
    assert got["dev_ratio"].tobytes() == ref.dev_ratio.tobytes() and got["npasses"] == ref.npasses
    assert R.rmock_unif_count() == 0 and R.rmock_protect_depth() == 0
