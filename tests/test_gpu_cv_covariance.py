"""Cross-validation in covariance mode: every fold fit of every alpha from ONE native call (sa.cv_covariance_fits ->
sgdnet_cv_covariance_*, sgdnet_amd/csrc/covariance.hip) and cv_sgdnet(fold_fits="batched") on top of it.

Fold fit (alpha, fold j) is BY DEFINITION sa.sgdnet(x[T], y[T], alpha=alpha, lambda_=lambda, mode="covariance") for the
training set T of fold j.  The primary check is independent of any solver: the optimality conditions of that problem on
x[T], y[T] (sa.kkt) within the project's bound, for every job and every lambda.  The second check is the separate fit
itself, to the project's figure for "the same optimum reached twice".

Tolerances
  KKT_BOUND = 1e-8          KKT residual <= 1e-8 * lambda: tests/test_gpu_covariance.py.
  SAME_OPTIMUM = 1e-9       relative to max|beta| (test_user_lambdas_need_not_be_monotone).  dev_ratio is held to it relative
                            to max|dev_ratio|.  a0 = mean_T(y) - sum_j mean_T(x_j) beta_j is held to it relative to the larger
                            of max|a0| and |mean_T(y)|, the size of what it is the difference of: without an intercept the
                            separate fit returns the mean of its standardised response, a rounding residue where this call
                            returns 0, and "relative to max|a0|" alone would compare two roundings.
  tests/test_cv_covariance_host.py measures what the pooling of the moments itself costs: <= 1.8e-14 in S and c~.

The shapes (n, p, folds) sit at the kernels' edges: groups of 65 rows (one past the 64-row stage), groups of exactly 64 with
p + 1 = 18 columns (across the 16-column tile), ten groups, and the largest p one workgroup's LDS holds.  Every training set
has more rows than features, so the lasso optimum is unique."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

KKT_BOUND = 1e-8
SAME_OPTIMUM = 1e-9
SHAPES = [(37, 2, 3), (195, 15, 3), (192, 17, 3), (1003, 33, 10), (1200, None, 3)]     # None: covariance_max_features()
NLAMBDA = 8
TIGHT = dict(thresh=1e-12, maxit=1_000_000)


def problem(n, p, sparse, seed=0):
    """tests/test_gpu_covariance.py problem(): columns of different means and scales (sparse: ~35 % stored), y = x B + noise"""
    rng = np.random.default_rng(1000 * seed + 7 * n + p)
    x = rng.standard_normal((n, p)) * rng.uniform(0.5, 3.0, p) + rng.uniform(-2.0, 2.0, p)
    if sparse:
        keep = rng.random((n, p)) < 0.35
        keep[0, :] = True
        x = x * keep
    B = rng.standard_normal(p) * (rng.random(p) < 0.5)
    y = x @ B + 0.5 * rng.standard_normal(n) + 1.5
    return (sp.csr_matrix(x) if sparse else x), y


def equal_folds(n, G, seed=0):
    """labels 1..G in random order, sizes as equal as n allows (exactly n / G where G divides n)"""
    return np.random.default_rng(seed).permutation(np.arange(n) % G) + 1


def training_sets(foldid, train_on):
    return [(foldid == v) == (train_on == "fold") for v in np.unique(foldid)]


def assert_optimal(k, lam, what):
    print(what, "ratio max %.3g intercept/lambda max %.3g" % (np.max(k["ratio"]), np.max(k["intercept"] / np.maximum(lam, 1e-300))))
    assert (k["ratio"] <= KKT_BOUND).all(), (what, k["ratio"])
    assert (k["intercept"] <= KKT_BOUND * lam).all(), (what, k["intercept"], lam)


def assert_same_fit(got, ref, y_mean, what):
    b = np.abs(got.beta - ref.beta).max() / np.abs(ref.beta).max()
    d = np.abs(got.dev_ratio - ref.dev_ratio).max() / np.abs(ref.dev_ratio).max()
    a = np.abs(got.a0 - ref.a0).max() / max(np.abs(ref.a0).max(), abs(y_mean))
    print(what, "vs the separate fit: beta %.3g dev_ratio %.3g a0 %.3g" % (b, d, a))
    assert b <= SAME_OPTIMUM and d <= SAME_OPTIMUM and a <= SAME_OPTIMUM, (what, b, d, a)
    assert got.nobs == ref.nobs and abs(got.nulldev - ref.nulldev) <= SAME_OPTIMUM * ref.nulldev


@pytest.fixture(scope="module")
def sa():
    import torch  # noqa: F401
    import sgdnet_amd
    if sgdnet_amd.load().sgdnet_device_count() < 1:
        pytest.fail("GPU tests need a HIP device; the backend has no CPU fallback")
    return sgdnet_amd


def check_jobs(sa, x, y, foldid, mixes, train_on, standardize=True, intercept=True, compare=True, nlambda=NLAMBDA, lambda_min_ratio=1e-2):
    """one batched call over `mixes`; KKT on x[T], y[T] for every job and lambda, and the separate fit of every job"""
    opts = dict(standardize=standardize, intercept=intercept, **TIGHT)
    lam = [sa.sgdnet(x, y, alpha=m, nlambda=nlambda, lambda_min_ratio=lambda_min_ratio, mode="covariance", **opts).lambda_ for m in mixes]
    fits = sa.cv_covariance_fits(x, y, foldid, mixes, lam, train_on=train_on, **opts)
    sets = training_sets(foldid, train_on)
    assert len(fits) == len(mixes) * len(sets)
    for a, m in enumerate(mixes):
        for j, T in enumerate(sets):
            fit, xT, yT = fits[a * len(sets) + j], x[T], y[T]
            what = (x.shape, sp.issparse(x), m, train_on, standardize, intercept, j)
            assert (fit.return_codes == 0).all() and fit.draws_used == 0 and fit.alpha == m, what
            assert np.array_equal(fit.lambda_, lam[a]) and np.isfinite(fit.dev_ratio).all()
            assert_optimal(sa.kkt(fit, xT, yT, standardize=standardize, intercept=intercept), fit.lambda_, what)     # no job, no lambda dropped
            if compare:
                ref = sa.sgdnet(xT, yT, alpha=m, lambda_=lam[a], mode="covariance", **opts)
                assert_same_fit(fit, ref, yT.mean(), what)
    return fits


# ---- 1. the envelope ----

@pytest.mark.parametrize("train_on", ["fold", "rest"])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_fold_fit_is_optimal_and_the_separate_fit(sa, shape, sparse, train_on):
    n, p, G = shape[0], shape[1] or sa.covariance_max_features(), shape[2]
    x, y = problem(n, p, sparse)
    mixes = [0.0, 0.5, 1.0]
    if shape[1] is None:
        # a path at the largest p takes a second at this thresh, and the separate fits run one after another: one mix per
        # case here, chosen so that the four cases of this shape still see all three
        mixes = [mixes[(2 * sparse + (train_on == "rest") + 1) % 3]]
    check_jobs(sa, x, y, equal_folds(n, G), mixes, train_on)


@pytest.mark.parametrize("train_on", ["fold", "rest"])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", SHAPES[:2])
def test_intercept_and_standardize_combinations(sa, shape, sparse, train_on):
    n, p, G = shape
    x, y = problem(n, p, sparse, seed=1)
    for intercept, standardize in ((True, False), (False, True), (False, False)):     # (True, True) is the test above
        check_jobs(sa, x, y, equal_folds(n, G, seed=1), [0.0, 0.5, 1.0], train_on, standardize=standardize, intercept=intercept)


# ---- 2. awkward folds ----

@pytest.mark.parametrize("sparse", [False, True])
def test_folds_cut_along_a_sorted_column(sa, sparse):
    """every fold's mean of column 0 sits far from the whole-data mean the group moments are centred at"""
    n, p, G = 195, 15, 3
    x, y = problem(n, p, sparse, seed=2)
    col = np.asarray(x[:, 0].todense()).ravel() if sparse else x[:, 0]
    foldid = np.empty(n, dtype=np.int64)
    foldid[np.argsort(col, kind="stable")] = np.arange(n) * G // n
    for train_on in ("fold", "rest"):
        check_jobs(sa, x, y, foldid, [0.5, 1.0], train_on)


@pytest.mark.parametrize("sparse", [False, True])
def test_unequal_groups_and_a_group_of_one(sa, sparse):
    n, p = 120, 5
    x, y = problem(n, p, sparse, seed=3)
    foldid = np.repeat([10, 20, 30, 40], [1, 19, 65, 35])          # labels need not be 1..G; a group of one row
    foldid = foldid[np.random.default_rng(3).permutation(n)]
    check_jobs(sa, x, y, foldid, [0.5, 1.0], "rest")
    keep = foldid != 10                                             # train_on="fold" cannot fit a single row's variance
    check_jobs(sa, x[keep], y[keep], foldid[keep], [0.5, 1.0], "fold")


@pytest.mark.parametrize("sparse", [False, True])
def test_leave_one_out(sa, sparse):
    n, p = 12, 2
    x, y = problem(n, p, sparse, seed=4)
    check_jobs(sa, x, y, np.arange(n), [0.5, 1.0], "rest")          # nfolds = n


@pytest.mark.parametrize("sparse", [False, True])
def test_large_mean_column(sa, sparse):
    """a column of mean 1e6 and sd 1 (every entry stored): KKT on x[T], y[T] only -- the separate fit centres the same
    column at another mean and the two share nothing but the optimum.
    The path is that of tests/test_gpu_covariance.py::test_large_mean_column_does_not_cancel (lambda_min_ratio = 0.05) for
    the reason it has it: the coefficient of that column is about 0.7, so a0 is about -7e5 and one unit in its last place is
    1.2e-10 -- the intercept's residual cannot be held below that, and KKT_BOUND * lambda has to stay above it (at 0.05 of
    lambda_max ~ 0.9 it is 4.6e-10; at 0.01 it would be 9e-11, below what an f64 a0 can express)."""
    n, p, G = 195, 5, 3
    x, y = problem(n, p, sparse, seed=5)
    xd = np.asarray(x.todense()) if sparse else x.copy()
    col = np.random.default_rng(11).standard_normal(n)
    xd[:, 2] = 1e6 + (col - col.mean()) / col.std()
    y = y + 0.7 * col
    x = sp.csr_matrix(xd) if sparse else xd
    for train_on in ("fold", "rest"):
        check_jobs(sa, x, y, equal_folds(n, G, seed=5), [0.5, 1.0], train_on, compare=False, nlambda=10, lambda_min_ratio=0.05)


# ---- 3. independence and determinism ----

@pytest.mark.parametrize("sparse", [False, True])
def test_jobs_are_independent_and_repeatable(sa, sparse):
    n, p, G = 1003, 33, 10
    x, y = problem(n, p, sparse, seed=6)
    foldid = equal_folds(n, G, seed=6)
    lam = np.geomspace(1.0, 0.01, 6)
    kw = dict(thresh=1e-9, maxit=100000)
    alone = sa.cv_covariance_fits(x, y, foldid, [0.5], [lam], **kw)
    among = sa.cv_covariance_fits(x, y, foldid, [0.2, 0.5, 1.0], [lam, lam, lam], **kw)
    again = sa.cv_covariance_fits(x, y, foldid, [0.2, 0.5, 1.0], [lam, lam, lam], **kw)
    for j in range(G):
        for name in ("beta", "a0", "dev_ratio", "return_codes"):
            assert getattr(alone[j], name).tobytes() == getattr(among[G + j], name).tobytes(), (j, name)
        assert alone[j].npasses == among[G + j].npasses > 0
    for f, g in zip(among, again):
        assert f.beta.tobytes() == g.beta.tobytes() and f.a0.tobytes() == g.a0.tobytes()
        assert f.dev_ratio.tobytes() == g.dev_ratio.tobytes() and f.npasses == g.npasses and f.nulldev == g.nulldev


def test_generator_ends_in_the_same_state(sa):
    x, y = problem(195, 15, False, seed=7)
    state, folds = [], []
    for fold_fits in ("separate", "batched"):
        rng = sa.RRng(3)
        cv = sa.cv_sgdnet(x, y, alpha=[0.5, 1.0], nfolds=3, rng=rng, nlambda=5, mode="covariance", fold_fits=fold_fits)
        state.append(bytes(rng.state))
        folds.append(cv.foldid)
    assert state[0] == state[1] and state[0] != bytes(sa.RRng(3).state)       # (sample() for the fold ids moved it)
    assert np.array_equal(folds[0], folds[1])


# ---- 4. cv_sgdnet on abalone ----

@pytest.mark.parametrize("train_on", ["fold", "rest"])
def test_cv_sgdnet_batched_is_the_separate_cv_on_abalone(sa, train_on):
    ab = np.load(os.path.join(GOLD, "abalone.npz"))
    kw = dict(alpha=[0.5, 1], nfolds=5, seed=1, train_on=train_on, mode="covariance", thresh=1e-12, maxit=1_000_000, nlambda=20)
    sep = sa.cv_sgdnet(ab["x"], ab["y"], fold_fits="separate", **kw)
    bat = sa.cv_sgdnet(ab["x"], ab["y"], fold_fits="batched", **kw)
    assert np.array_equal(sep.foldid, bat.foldid) and sep.name == bat.name
    assert sep.cv_summary.shape == bat.cv_summary.shape and np.array_equal(sep.cv_summary[:, :2], bat.cv_summary[:, :2])
    for a, b in zip(sep.lambda_, bat.lambda_):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(sep.cv_raw, bat.cv_raw):
        err = np.abs(a - b).max() / np.abs(a).max()
        print("abalone %s: cv_raw batched vs separate, relative %.3g" % (train_on, err))
        assert err <= SAME_OPTIMUM
    assert (sep.alpha_min, sep.lambda_min, sep.lambda_1se) == (bat.alpha_min, bat.lambda_min, bat.lambda_1se)
    assert sep.fit.beta.tobytes() == bat.fit.beta.tobytes()


# ---- 5. refusals ----

def test_refusals_name_the_condition(sa):
    rng = np.random.default_rng(0)
    x = rng.standard_normal((60, 4))
    y = x[:, 0] + rng.standard_normal(60)
    fold = np.arange(60) % 3
    pm = sa.covariance_max_features()

    def refused(code, needle, xx, yy, ff):
        with pytest.raises(sa.SgdnetError) as e:
            sa.cv_covariance_fits(xx, yy, ff, 0.5, [0.1, 0.01])
        assert e.value.code == code and needle in str(e.value), str(e.value)

    wide = rng.standard_normal((30, pm + 1))
    refused(-5, "mode = covariance needs no more features than sgdnet_covariance_max_features()", wide, wide[:, 0], np.arange(30) % 3)
    refused(-5, "mode = covariance needs no more features", sp.csc_matrix(wide), wide[:, 0], np.arange(30) % 3)
    big = rng.standard_normal((300, pm))
    refused(-5, "mode = covariance needs the group moments within", big, big[:, 0], np.arange(300))
    for needle, kw in (("mode='covariance'", dict(mode="auto")), ("mode='covariance'", dict()),
                       ("family='gaussian'", dict(mode="covariance", family="binomial")),
                       ("one device", dict(mode="covariance", devices=[0, 0])),
                       ("debug", dict(mode="covariance", debug=True))):
        with pytest.raises(ValueError) as e:
            sa.cv_sgdnet(x, (y > 0).astype(float) if kw.get("family") else y, nfolds=3, fold_fits="batched", **kw)
        assert needle in str(e.value), str(e.value)
    # (n_gpus, debug, fold ids, empty groups and negative lambdas at the C ABI: tests/test_cv_covariance_host.py, no device needed)
    # ... and no other mode is touched: a mode="auto" CV still draws samples
    rng_state = sa.RRng(2)
    cv = sa.cv_sgdnet(x, y, nfolds=3, nlambda=3, mode="auto", rng=rng_state, foldid=fold + 1)
    assert cv.fit.draws_used > 0 and bytes(rng_state.state) != bytes(sa.RRng(2).state)
