"""Cross-validation in multi-response covariance mode: every fold fit of every alpha of an mgaussian CV from ONE native call
(sa.cv_mcovariance_fits -> sgdnet_cv_mcovariance_*, sgdnet_amd/csrc/covariance.hip: mcovariance_cv_run) and
sa.cv_sgdnet_mcovariance(fold_fits="batched") on top of it.

Fold fit (alpha, fold j) is BY DEFINITION sa.sgdnet_mcovariance(x[T], y[T], alpha=alpha, lambda_=lambda) for the training
set T of fold j.  The pass/fail check is independent of any solver: the optimality conditions of that problem on x[T], y[T]
(sa.kkt) within the project's bound, for every job and every lambda -- at 0 < alpha < 1 there is nothing else to compare
with.  The second check is the separate fit itself, to the project's figure for "the same optimum reached twice".

Tolerances
  KKT_BOUND = 1e-8          KKT ratio <= 1e-8, intercept residual <= 1e-8 * lambda: tests/test_gpu_mcovariance.py,
                            tests/test_gpu_cv_covariance.py.
  SAME_OPTIMUM = 1e-9       tests/test_gpu_cv_covariance.py: beta relative to max|beta|, dev_ratio to max|dev_ratio|, a0 to the
                            larger of max|a0| and max_r |mean_T(y_r)| (with standardize_response, or without an intercept, the
                            separate fit returns means of a standardised response, a rounding residue where this call returns
                            0).  nulldev within 1e-9 relative, nobs equal.
  tests/test_cv_mcovariance_host.py measures what the pooling of the K-response moments itself costs in S and c~.

The shapes (n, p, K, folds) sit at the kernels' edges; every training set has more rows than features in both train_on
modes, so the group-lasso optimum is unique at alpha = 1:
  (37, 2, 3, 3)       the smallest
  (120, 16, 4, 3)     p K = 64: the last shape of the one-wavefront path kernel
  (195, 13, 5, 3)     groups of 65 rows, one past the 64-row stage; p K = 65: the 256-lane kernel; the augmented columns 13..17
                      are the responses across the 16-column tile edge, the ones column is 18
  (192, 14, 2, 3)     groups of exactly 64; p + K + 1 = 17: the ones column alone in the second tile
  (1003, 33, 3, 10)   ten groups
  (1200, max, 2, 3), (1200, max, 10, 3), (600, max, 96, 3)    the feature limit of K = 2, 10, 96 (195, 174, 63)

The width of the path kernel's workgroup (64 / 256 lanes) is a constant of the shipped library (SGDNET_MCOV_WIDTH exists in
-DSGDNET_EXPERIMENTS builds only), so there is no width to select here: p K = 64 and p K = 65 above run one each.

Seen on an MI355X over all cases: worst KKT ratio 6.7e-11 and intercept residual 1.6e-13 lambda (3.8e-10 and 1.6e-9 lambda at
the column of mean 1e6); against the separate fit beta 6.4e-15, dev_ratio 2.2e-13, a0 1.5e-14; cv_raw 1.1e-15."""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

KKT_BOUND = 1e-8
SAME_OPTIMUM = 1e-9
SHAPES = [(37, 2, 3, 3), (120, 16, 4, 3), (195, 13, 5, 3), (192, 14, 2, 3), (1003, 33, 3, 10)]
LIMIT_SHAPES = [(1200, 2, 3), (1200, 10, 3), (600, 96, 3)]      # (n, K, folds); p = sa.mcovariance_max_features(K)
MIXES = [0.0, 0.5, 1.0]
NLAMBDA = 8
TIGHT = dict(thresh=1e-12, maxit=1_000_000)


def problem(n, p, K, sparse, seed=0):
    """tests/test_gpu_mcovariance.py problem(): x with columns of different means and scales (sparse: ~35 % stored, the
    first row always), y = x B + noise with half of B's rows zero and a different mean per response."""
    rng = np.random.default_rng(1000 * seed + 7 * n + 31 * p + K)
    x = rng.standard_normal((n, p)) * rng.uniform(0.5, 3.0, p) + rng.uniform(-2.0, 2.0, p)
    if sparse:
        keep = rng.random((n, p)) < 0.35
        keep[0, :] = True
        x = x * keep
    B = rng.standard_normal((p, K)) * (rng.random(p) < 0.5)[:, None]
    y = x @ B + 0.5 * rng.standard_normal((n, K)) * rng.uniform(0.5, 2.0, K) + rng.uniform(-2.0, 2.0, K)
    return (sp.csr_matrix(x) if sparse else x), y


def equal_folds(n, G, seed=0):
    """labels 1..G in random order, sizes as equal as n allows (exactly n / G where G divides n)"""
    return np.random.default_rng(seed).permutation(np.arange(n) % G) + 1


def training_sets(foldid, train_on):
    return [(foldid == v) == (train_on == "fold") for v in np.unique(foldid)]


def stacked(fit):
    return np.stack([np.asarray(b) for b in fit.beta])              # (K, p, L)


def assert_optimal(k, lam, what):
    print(what, "ratio max %.3g intercept/lambda max %.3g" % (np.max(k["ratio"]), np.max(k["intercept"] / np.maximum(lam, 1e-300))))
    assert (k["ratio"] <= KKT_BOUND).all(), (what, k["ratio"])
    assert (k["intercept"] <= KKT_BOUND * lam).all(), (what, k["intercept"], lam)


def assert_same_fit(got, ref, y_means, what):
    gb, rb = stacked(got), stacked(ref)
    assert gb.shape == rb.shape and got.a0.shape == ref.a0.shape and got.grouped and ref.grouped and got.family == ref.family == "mgaussian"
    b = np.abs(gb - rb).max() / np.abs(rb).max()
    d = np.abs(got.dev_ratio - ref.dev_ratio).max() / np.abs(ref.dev_ratio).max()
    a = np.abs(got.a0 - ref.a0).max() / max(np.abs(ref.a0).max(), np.abs(y_means).max())
    print(what, "vs the separate fit: beta %.3g dev_ratio %.3g a0 %.3g" % (b, d, a))
    assert b <= SAME_OPTIMUM and d <= SAME_OPTIMUM and a <= SAME_OPTIMUM, (what, b, d, a)
    assert got.nobs == ref.nobs and abs(got.nulldev - ref.nulldev) <= SAME_OPTIMUM * ref.nulldev
    assert np.array_equal(got.df, ref.df) and np.array_equal(got.dfmat, ref.dfmat)


@pytest.fixture(scope="module")
def sa():
    import torch  # noqa: F401
    import sgdnet_amd
    if sgdnet_amd.load().sgdnet_device_count() < 1:
        pytest.fail("GPU tests need a HIP device; the backend has no CPU fallback")
    return sgdnet_amd


def check_jobs(sa, x, y, foldid, mixes, train_on, standardize=True, intercept=True, standardize_response=False, compare=True,
               nlambda=NLAMBDA, lambda_min_ratio=1e-2):
    """one batched call over `mixes`; KKT on x[T], y[T] for every job and lambda, and the separate fit of every job"""
    opts = dict(standardize=standardize, intercept=intercept, standardize_response=standardize_response, **TIGHT)
    lam = [sa.sgdnet_mcovariance(x, y, alpha=m, nlambda=nlambda, lambda_min_ratio=lambda_min_ratio, **opts).lambda_ for m in mixes]
    fits = sa.cv_mcovariance_fits(x, y, foldid, mixes, lam, train_on=train_on, **opts)
    sets = training_sets(foldid, train_on)
    assert len(fits) == len(mixes) * len(sets)
    for a, m in enumerate(mixes):
        for j, T in enumerate(sets):
            fit, xT, yT = fits[a * len(sets) + j], x[T], y[T]
            what = (x.shape, y.shape[1], sp.issparse(x), m, train_on, standardize, intercept, standardize_response, j)
            assert (fit.return_codes == 0).all() and fit.draws_used == 0 and fit.alpha == m, what
            assert np.array_equal(fit.lambda_, lam[a]) and np.isfinite(fit.dev_ratio).all() and fit.npasses > 0
            k = sa.kkt(fit, xT, yT, standardize=standardize, intercept=intercept, standardize_response=standardize_response)
            assert_optimal(k, fit.lambda_, what)                                    # no job, no lambda dropped
            if compare:
                ref = sa.sgdnet_mcovariance(xT, yT, alpha=m, lambda_=lam[a], **opts)
                assert_same_fit(fit, ref, yT.mean(axis=0), what)
    return fits


# ---- 1. the envelope ----

@pytest.mark.parametrize("train_on", ["fold", "rest"])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_fold_fit_is_optimal_and_the_separate_fit(sa, shape, sparse, train_on):
    n, p, K, G = shape
    x, y = problem(n, p, K, sparse)
    check_jobs(sa, x, y, equal_folds(n, G), MIXES, train_on)


@pytest.mark.parametrize("train_on", ["fold", "rest"])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", LIMIT_SHAPES)
def test_fold_fits_at_the_feature_limit(sa, shape, sparse, train_on):
    """a path at the largest p takes a while at this thresh and the separate fits run one after another: one mix per case,
    chosen so that the four cases of a shape still see all three"""
    n, K, G = shape
    p = sa.mcovariance_max_features(K)
    x, y = problem(n, p, K, sparse)
    check_jobs(sa, x, y, equal_folds(n, G), [MIXES[(2 * sparse + (train_on == "rest") + 1) % 3]], train_on)


@pytest.mark.parametrize("train_on", ["fold", "rest"])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", SHAPES[:3])
def test_intercept_and_standardize_combinations(sa, shape, sparse, train_on):
    n, p, K, G = shape
    x, y = problem(n, p, K, sparse, seed=1)
    for intercept, standardize in ((True, False), (False, True), (False, False)):     # (True, True) is the test above
        check_jobs(sa, x, y, equal_folds(n, G, seed=1), MIXES, train_on, standardize=standardize, intercept=intercept)


@pytest.mark.parametrize("train_on", ["fold", "rest"])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", SHAPES[:3])
def test_standardize_response(sa, shape, sparse, train_on):
    n, p, K, G = shape
    x, y = problem(n, p, K, sparse, seed=2)
    check_jobs(sa, x, y, equal_folds(n, G, seed=2), MIXES, train_on, standardize_response=True)


# ---- 2. awkward folds ----

@pytest.mark.parametrize("sparse", [False, True])
def test_folds_cut_along_a_sorted_column(sa, sparse):
    """every fold's mean of column 0 sits far from the whole-data mean the group moments are centred at"""
    n, p, K, G = 195, 13, 5, 3
    x, y = problem(n, p, K, sparse, seed=3)
    col = np.asarray(x[:, 0].todense()).ravel() if sparse else x[:, 0]
    foldid = np.empty(n, dtype=np.int64)
    foldid[np.argsort(col, kind="stable")] = np.arange(n) * G // n
    for train_on in ("fold", "rest"):
        check_jobs(sa, x, y, foldid, [0.5, 1.0], train_on)


@pytest.mark.parametrize("sparse", [False, True])
def test_unequal_groups_and_a_group_of_one(sa, sparse):
    n, p, K = 120, 5, 3
    x, y = problem(n, p, K, sparse, seed=4)
    foldid = np.repeat([10, 20, 30, 40], [1, 19, 65, 35])          # labels need not be 1..G; a group of one row
    foldid = foldid[np.random.default_rng(3).permutation(n)]
    check_jobs(sa, x, y, foldid, [0.5, 1.0], "rest")
    keep = foldid != 10                                             # train_on="fold" cannot fit a single row's variance
    check_jobs(sa, x[keep], y[keep], foldid[keep], [0.5, 1.0], "fold")


@pytest.mark.parametrize("sparse", [False, True])
def test_leave_one_out(sa, sparse):
    n, p, K = 37, 2, 3
    x, y = problem(n, p, K, sparse, seed=5)
    check_jobs(sa, x, y, np.arange(n), [0.5, 1.0], "rest")          # nfolds = n


@pytest.mark.parametrize("sparse", [False, True])
def test_large_mean_column(sa, sparse):
    """a column of mean 1e6 and sd 1 (every entry stored): KKT on x[T], y[T] only, on the path of
    tests/test_gpu_cv_covariance.py::test_large_mean_column for the reason given there (the intercepts are of the order of
    7e5, one unit in their last place is 1.2e-10, and KKT_BOUND * lambda has to stay above it)."""
    n, p, K, G = 195, 5, 3, 3
    x, y = problem(n, p, K, sparse, seed=6)
    xd = np.asarray(x.todense()) if sparse else x.copy()
    col = np.random.default_rng(11).standard_normal(n)
    xd[:, 2] = 1e6 + (col - col.mean()) / col.std()
    y = y + 0.7 * col[:, None]
    x = sp.csr_matrix(xd) if sparse else xd
    for train_on in ("fold", "rest"):
        check_jobs(sa, x, y, equal_folds(n, G, seed=6), [0.5, 1.0], train_on, compare=False, nlambda=10, lambda_min_ratio=0.05)


# ---- 3. independence and determinism ----

@pytest.mark.parametrize("sparse", [False, True])
def test_jobs_are_independent_and_repeatable(sa, sparse):
    n, p, K, G = 1003, 33, 3, 10
    x, y = problem(n, p, K, sparse, seed=7)
    foldid = equal_folds(n, G, seed=7)
    lam = np.geomspace(1.0, 0.01, 6)
    kw = dict(thresh=1e-9, maxit=100000)
    alone = sa.cv_mcovariance_fits(x, y, foldid, [0.5], [lam], **kw)
    among = sa.cv_mcovariance_fits(x, y, foldid, MIXES, [lam, lam, lam], **kw)
    again = sa.cv_mcovariance_fits(x, y, foldid, MIXES, [lam, lam, lam], **kw)
    for j in range(G):
        assert stacked(alone[j]).tobytes() == stacked(among[G + j]).tobytes(), j
        for name in ("a0", "dev_ratio", "return_codes"):
            assert getattr(alone[j], name).tobytes() == getattr(among[G + j], name).tobytes(), (j, name)
        assert alone[j].npasses == among[G + j].npasses > 0
    for f, g in zip(among, again):
        assert stacked(f).tobytes() == stacked(g).tobytes() and f.a0.tobytes() == g.a0.tobytes()
        assert f.dev_ratio.tobytes() == g.dev_ratio.tobytes() and f.npasses == g.npasses and f.nulldev == g.nulldev


# ---- 4. cv_sgdnet_mcovariance ----

@pytest.mark.parametrize("train_on", ["fold", "rest"])
def test_cv_batched_is_the_separate_cv(sa, train_on):
    x, y = problem(400, 9, 3, False)
    kw = dict(alpha=[0.5, 1], nfolds=5, train_on=train_on, nlambda=20, **TIGHT)
    cvs, states = [], []
    for fold_fits in ("separate", "batched"):
        rng = sa.RRng(3)
        cvs.append(sa.cv_sgdnet_mcovariance(x, y, fold_fits=fold_fits, rng=rng, **kw))
        states.append(bytes(rng.state))
    sep, bat = cvs
    assert states[0] == states[1] and states[0] != bytes(sa.RRng(3).state)     # (sample() for the fold ids moved it)
    assert np.array_equal(sep.foldid, bat.foldid) and sep.name == bat.name
    assert sep.cv_summary.shape == bat.cv_summary.shape and np.array_equal(sep.cv_summary[:, :2], bat.cv_summary[:, :2])
    for a, b in zip(sep.lambda_, bat.lambda_):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(sep.cv_raw, bat.cv_raw):
        err = np.abs(a - b).max() / np.abs(a).max()
        print("%s: cv_raw batched vs separate, relative %.3g" % (train_on, err))
        assert err <= SAME_OPTIMUM
    assert (sep.alpha_min, sep.lambda_min) == (bat.alpha_min, bat.lambda_min)
    assert stacked(sep.fit).tobytes() == stacked(bat.fit).tobytes()


# ---- 5. refusals ----

def test_refusals_name_the_condition(sa):
    rng = np.random.default_rng(0)
    x = rng.standard_normal((60, 4))
    y = x[:, :3] + rng.standard_normal((60, 3))

    def refused(code, needle, xx, yy, ff):
        with pytest.raises(sa.SgdnetError) as e:
            sa.cv_mcovariance_fits(xx, yy, ff, 0.5, [0.1, 0.01])
        assert e.value.code == code and needle in str(e.value), str(e.value)

    pm = sa.mcovariance_max_features(3)
    wide = rng.standard_normal((30, pm + 1))
    refused(-5, "mode = mcovariance needs no more features than sgdnet_mcovariance_max_features(n_classes)", wide, wide[:, :3],
            np.arange(30) % 3)
    refused(-5, "mode = mcovariance needs no more features", sp.csc_matrix(wide), wide[:, :3], np.arange(30) % 3)
    big = rng.standard_normal((300, pm))
    refused(-5, "mode = mcovariance needs the group moments within", big, big[:, :3], np.arange(300))
    with pytest.raises(ValueError):
        sa.cv_sgdnet_mcovariance(x, y, nfolds=3, fold_fits="fused")
    # (family, n_classes, n_gpus, debug, fold ids, empty groups and negative lambdas at the C ABI:
    #  tests/test_cv_mcovariance_host.py, no device needed)
    # ... and the refusing call left the device usable
    fits = sa.cv_mcovariance_fits(x, y, np.arange(60) % 3, 0.5, [0.1, 0.01])
    assert len(fits) == 3 and all((f.return_codes == 0).all() for f in fits)
