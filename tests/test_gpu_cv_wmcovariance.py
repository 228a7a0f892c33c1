"""Cross-validation in wide multi-response covariance mode: every fold fit of every alpha of an mgaussian CV from ONE native
call (sa.cv_wmcovariance_fits -> sgdnet_cv_wmcovariance_*, sgdnet_amd/csrc/covariance.hip: wmcovariance_cv_run) and
sa.cv_sgdnet_wmcovariance(fold_fits="batched").

Fold fit (alpha, fold j) is BY DEFINITION sa.sgdnet_wmcovariance(x[T], y[T], alpha=alpha, lambda_=lambda) for the training
set T of fold j.  The primary check is independent of any solver: the optimality conditions of that problem on x[T], y[T]
(sa.kkt) within the project's bound, for every job and every lambda, none dropped.  The second check is the separate fit
itself, to the project's figure for "the same optimum reached twice", wherever the optimum is unique: the training set has
more rows than features, or the mix is below 1.  Inputs, shapes and tolerances: tests/cv_wmcovariance_reference.py.

Seen on an MI355X over all cases: worst KKT ratio 3.0e-10 and intercept residual 2.0e-13 lambda (2.4e-10 and 3.9e-9 lambda at
the column of mean 1e6); against the separate fit beta 8.8e-13, dev_ratio 6.4e-14, a0 6.7e-13, and against the narrow CV at
its limit (600, 195, 2) beta 1.4e-11, dev_ratio 5.7e-14, a0 2.0e-11 (two different descents stopped at thresh); cv_raw
1.3e-15."""
import numpy as np
import pytest
import scipy.sparse as sp

import cv_wmcovariance_reference as cr
import test_gpu_cv_mcovariance as tcm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sa():
    import torch  # noqa: F401
    import sgdnet_amd
    if sgdnet_amd.load().sgdnet_device_count() < 1:
        pytest.fail("GPU tests need a HIP device; the backend has no CPU fallback")
    return sgdnet_amd


def same_bytes(f, g):
    return tcm.stacked(f).tobytes() == tcm.stacked(g).tobytes() and \
        all(getattr(f, name).tobytes() == getattr(g, name).tobytes() for name in ("a0", "dev_ratio", "return_codes")) and \
        f.npasses == g.npasses and f.nulldev == g.nulldev


def check_lambdas(sa, x, y, foldid, mixes, lam, train_on, opts, compare=True):
    """one batched call over `mixes`; KKT on x[T], y[T] for every job and lambda, and the separate fit of every job whose
    optimum is unique"""
    standardize, intercept, std_y = opts["standardize"], opts["intercept"], opts["standardize_response"]
    fits = sa.cv_wmcovariance_fits(x, y, foldid, mixes, lam, train_on=train_on, **opts)
    sets = cr.training_sets(foldid, train_on)
    assert len(fits) == len(mixes) * len(sets)
    for a, m in enumerate(mixes):
        for j, T in enumerate(sets):
            fit, xT, yT = fits[a * len(sets) + j], x[T], y[T]
            what = (x.shape, y.shape[1], sp.issparse(x), m, train_on, standardize, intercept, std_y, j)
            assert (fit.return_codes == 0).all() and fit.draws_used == 0 and fit.alpha == m and fit.npasses > 0, (what, fit.return_codes)
            assert np.array_equal(fit.lambda_, lam[a]) and np.isfinite(fit.dev_ratio).all() and fit.nobs == T.sum()
            k = sa.kkt(fit, xT, yT, standardize=standardize, intercept=intercept, standardize_response=std_y)
            tcm.assert_optimal(k, fit.lambda_, what)                                # no job, no lambda dropped
            if compare and (T.sum() > x.shape[1] or m < 1.0):
                ref = sa.sgdnet_wmcovariance(xT, yT, alpha=m, lambda_=lam[a], **opts)
                assert (ref.return_codes == 0).all()
                tcm.assert_same_fit(fit, ref, yT.mean(axis=0), what)
    return fits


def check_jobs(sa, x, y, foldid, mixes, train_on, standardize=True, intercept=True, standardize_response=False, compare=True,
               nlambda=6, lambda_min_ratio=1e-2):
    opts = dict(standardize=standardize, intercept=intercept, standardize_response=standardize_response, **cr.TIGHT)
    lam = [cr.lambdas(x, y, m, standardize, nlambda, lambda_min_ratio, standardize_response) for m in mixes]
    return check_lambdas(sa, x, y, foldid, mixes, lam, train_on, opts, compare)


def path_kw(n, p, G):
    nlambda, ratio = cr.path_of(n, p, G)
    return dict(nlambda=nlambda, lambda_min_ratio=ratio)


# ---- 1. the envelope ----

@pytest.mark.parametrize("train_on", ["fold", "rest"])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", cr.SHAPES)
def test_every_fold_fit_is_optimal_and_the_separate_fit(sa, shape, sparse, train_on):
    n, p, K, G = shape
    x, y = cr.problem(n, p, K, sparse)
    mixes = cr.MIXES
    if p == 1025:
        # one mix per case, chosen so that the four cases of this shape see all three
        mixes = [mixes[(2 * sparse + (train_on == "rest") + 1) % 3]]
    check_jobs(sa, x, y, cr.equal_folds(n, G), mixes, train_on, **path_kw(n, p, G))


@pytest.mark.parametrize("train_on", ["fold", "rest"])
@pytest.mark.parametrize("shape", cr.LIMIT_SHAPES)
def test_fold_fits_at_the_feature_limit(sa, shape, train_on):
    n, K, G = shape
    p = sa.wmcovariance_max_features(K)
    assert p == cr.LIMITS[K]
    x, y = cr.problem(n, p, K, False)
    nlambda, ratio = cr.LIMIT_PATH
    check_jobs(sa, x, y, cr.equal_folds(n, G), [0.5], train_on, nlambda=nlambda, lambda_min_ratio=ratio)


@pytest.mark.parametrize("train_on", ["fold", "rest"])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", cr.NARROW_SHAPES)
def test_same_optimum_as_the_narrow_cv(sa, shape, sparse, train_on):
    n, p, K, G = shape
    x, y = cr.problem(n, p, K, sparse, seed=8)
    foldid = cr.equal_folds(n, G, seed=8)
    lam = [cr.lambdas(x, y, m, True, 6, 1e-2) for m in cr.MIXES]
    wide = sa.cv_wmcovariance_fits(x, y, foldid, cr.MIXES, lam, train_on=train_on, **cr.TIGHT)
    narrow = sa.cv_mcovariance_fits(x, y, foldid, cr.MIXES, lam, train_on=train_on, **cr.TIGHT)
    assert len(wide) == len(narrow) == 3 * G
    sets = cr.training_sets(foldid, train_on)
    for job, (w, c) in enumerate(zip(wide, narrow)):
        assert (w.return_codes == 0).all() and (c.return_codes == 0).all()
        tcm.assert_same_fit(w, c, y[sets[job % G]].mean(axis=0), (shape, sparse, train_on, job))


SETTING_SHAPES = [(195, 13, 5, 3), cr.FIRST_REFUSED]


@pytest.mark.parametrize("train_on", ["fold", "rest"])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("intercept,standardize", [(True, False), (False, True), (False, False)])     # (True, True) is the test above
@pytest.mark.parametrize("mix", cr.MIXES)          # (a case per mix: at 196 unscaled features a path takes a second at this thresh)
@pytest.mark.parametrize("shape", SETTING_SHAPES)
def test_intercept_and_standardize_combinations(sa, shape, mix, intercept, standardize, sparse, train_on):
    n, p, K, G = shape
    x, y = cr.problem(n, p, K, sparse, seed=1)
    check_jobs(sa, x, y, cr.equal_folds(n, G, seed=1), [mix], train_on, standardize=standardize, intercept=intercept)


@pytest.mark.parametrize("train_on", ["fold", "rest"])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", SETTING_SHAPES)
def test_standardize_response(sa, shape, sparse, train_on):
    n, p, K, G = shape
    x, y = cr.problem(n, p, K, sparse, seed=2)
    check_jobs(sa, x, y, cr.equal_folds(n, G, seed=2), cr.MIXES, train_on, standardize_response=True)


# ---- 2. awkward folds at the first p the narrow CV refuses (KKT only) ----

@pytest.mark.parametrize("sparse", [False, True])
def test_folds_cut_along_a_sorted_column(sa, sparse):
    n, p, K, G = cr.FIRST_REFUSED
    x, y = cr.problem(n, p, K, sparse, seed=2)
    for train_on in ("fold", "rest"):
        check_jobs(sa, x, y, cr.sorted_folds(x, G), [0.5, 1.0], train_on, compare=False)


@pytest.mark.parametrize("sparse", [False, True])
def test_unequal_groups_a_group_of_one_and_labels_that_are_not_1_to_G(sa, sparse):
    n, p, K, _ = cr.FIRST_REFUSED
    x, y = cr.problem(n, p, K, sparse, seed=3)
    foldid = cr.unequal_folds(n)
    assert sorted(np.bincount(foldid)[[10, 20, 30, 40]]) == [1, 199, 200, 200]
    check_jobs(sa, x, y, foldid, [0.5, 1.0], "rest", compare=False)      # (train_on="fold" cannot fit a single row's variance)


@pytest.mark.parametrize("sparse", [False, True])
def test_large_mean_column(sa, sparse):
    """a column of mean 1e6 and sd 1: on the path of tests/test_gpu_cv_covariance.py::test_large_mean_column (lambda_min_ratio =
    0.05) and for its reason -- the intercepts are of the order of 7e5, one unit in their last place is 1.2e-10, and
    KKT_BOUND * lambda has to stay above what an f64 a0 can express"""
    n, p, K, G = cr.FIRST_REFUSED
    x, y = cr.large_mean_problem(n, p, K, sparse)
    for train_on in ("fold", "rest"):
        check_jobs(sa, x, y, cr.equal_folds(n, G, seed=5), [0.5, 1.0], train_on, compare=False, **cr.LARGE_MEAN_PATH)


# ---- 3. more jobs than compute units ----

def test_more_jobs_than_compute_units(sa):
    n, p, K, G = cr.MANY_JOBS
    x, y = cr.problem(n, p, K, False, seed=4)
    fits = check_jobs(sa, x, y, np.arange(n), cr.MIXES, "rest")          # leave-one-out: every job optimal and its separate fit
    assert len(fits) == 270 > 256


# ---- 4. independence and determinism ----

@pytest.mark.parametrize("sparse", [False, True])
def test_jobs_are_independent_and_repeatable(sa, sparse):
    n, p, K, G = cr.FIRST_REFUSED
    x, y = cr.problem(n, p, K, sparse, seed=6)
    foldid = cr.equal_folds(n, G, seed=6)
    lam = np.geomspace(1.0, 0.01, 6)
    kw = dict(thresh=1e-9, maxit=100000)
    alone = sa.cv_wmcovariance_fits(x, y, foldid, [0.5], [lam], **kw)
    among = sa.cv_wmcovariance_fits(x, y, foldid, [0.2, 0.5, 1.0], [lam, lam, lam], **kw)
    again = sa.cv_wmcovariance_fits(x, y, foldid, [0.2, 0.5, 1.0], [lam, lam, lam], **kw)
    for j in range(G):
        assert same_bytes(alone[j], among[G + j]) and alone[j].npasses > 0, j
    for f, g in zip(among, again):
        assert same_bytes(f, g)


@pytest.mark.parametrize("shape", [cr.FIRST_REFUSED, (130, 1025, 3, 2)])
def test_both_widths_give_the_same_bits(sa, shape):
    n, p, K, G = shape
    x, y = cr.problem(n, p, K, False, seed=7)
    foldid = cr.equal_folds(n, G, seed=7)
    lam = [cr.lambdas(x, y, m, True, *cr.path_of(n, p, G)) for m in (0.5, 1.0)]
    kw = dict(train_on="rest", **cr.TIGHT)
    with sa.option("wmcovariance_width", 256):
        narrow = sa.cv_wmcovariance_fits(x, y, foldid, [0.5, 1.0], lam, **kw)
    with sa.option("wmcovariance_width", 1024):
        wide = sa.cv_wmcovariance_fits(x, y, foldid, [0.5, 1.0], lam, **kw)
    for f, g in zip(narrow, wide):
        assert same_bytes(f, g) and (f.return_codes == 0).all() and f.npasses > 0
    with sa.option("wmcovariance_width", 512):                 # not a width the library has
        with pytest.raises(sa.SgdnetError) as e:
            sa.cv_wmcovariance_fits(x, y, foldid, [0.5, 1.0], lam, **kw)
    assert e.value.code == -1


def test_max_iter_is_reported_per_job_and_lambda(sa):
    n, p, K, G = cr.FIRST_REFUSED
    x, y = cr.problem(n, p, K, False, seed=2)
    lam = [cr.lambdas(x, y, m, True, 5, 1e-2) for m in (0.5, 1.0)]
    fits = sa.cv_wmcovariance_fits(x, y, cr.equal_folds(n, G), [0.5, 1.0], lam, thresh=1e-14, maxit=2)
    assert len(fits) == 2 * G
    for fit in fits:
        # below lambda_max no two sweeps change the coefficients by less than 1e-14 of their size
        # (tests/test_gpu_wmcovariance.py::test_max_iter_is_reported)
        assert fit.npasses <= 2 * 5 and (fit.return_codes[1:] == 1).all(), fit.return_codes


# ---- 5. cv_sgdnet_wmcovariance ----

@pytest.mark.parametrize("train_on", ["fold", "rest"])
def test_cv_sgdnet_wmcovariance_batched_is_the_separate_cv(sa, train_on):
    n, p, K, _ = cr.FIRST_REFUSED
    x, y = cr.problem(n, p, K, False)
    state, cvs = [], []
    for fold_fits in ("separate", "batched"):
        rng = sa.RRng(3)
        cvs.append(sa.cv_sgdnet_wmcovariance(x, y, alpha=[0.5, 1], nfolds=3, rng=rng, train_on=train_on, nlambda=8, lambda_min_ratio=1e-2,
                                             fold_fits=fold_fits, **cr.TIGHT))
        state.append(bytes(rng.state))
    sep, bat = cvs
    assert state[0] == state[1] and state[0] != bytes(sa.RRng(3).state)       # (sample() for the fold ids moved it)
    assert np.array_equal(sep.foldid, bat.foldid) and sep.name == bat.name
    assert sep.cv_summary.shape == bat.cv_summary.shape and np.array_equal(sep.cv_summary[:, :2], bat.cv_summary[:, :2])
    for a, b in zip(sep.lambda_, bat.lambda_):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(sep.cv_raw, bat.cv_raw):
        err = np.abs(a - b).max() / np.abs(a).max()
        print("%s: cv_raw batched vs separate, relative %.3g" % (train_on, err))
        assert err <= cr.SAME_OPTIMUM
    assert (sep.alpha_min, sep.lambda_min, sep.lambda_1se) == (bat.alpha_min, bat.lambda_min, bat.lambda_1se)
    assert tcm.stacked(sep.fit).tobytes() == tcm.stacked(bat.fit).tobytes() and sep.fit.a0.tobytes() == bat.fit.a0.tobytes()


# ---- 6. refusals ----

def test_refusals_name_the_condition(sa):
    rng = np.random.default_rng(0)
    limit = sa.wmcovariance_max_features(2)

    def refused(fits, code, needle, xx, yy, ff):
        with pytest.raises(sa.SgdnetError) as e:
            fits(xx, yy, ff, 0.5, [0.1, 0.01])
        assert e.value.code == code and needle in str(e.value), str(e.value)

    wide = rng.standard_normal((6, limit + 1))
    refused(sa.cv_wmcovariance_fits, -5, "mode = wmcovariance needs no more features than sgdnet_wmcovariance_max_features(n_classes)", wide,
            wide[:, :2], np.arange(6) % 3)
    refused(sa.cv_wmcovariance_fits, -5, "mode = wmcovariance needs no more features", sp.csc_matrix(wide), wide[:, :2], np.arange(6) % 3)
    # the byte budget: enough groups of one row at a p where x itself stays small (6.8 MB)
    p = 1000
    G = cr.groups_over_budget(p, 2)
    big = rng.standard_normal((G, p))
    refused(sa.cv_wmcovariance_fits, -5,
            "mode = wmcovariance needs the moments and the scaled matrices of the groups within %d bytes" % cr.BUDGET_BYTES, big, big[:, :2],
            np.arange(G))
    # K = 1: cv_wmcovariance_fits refuses a one-column response itself; the library by its condition
    import ctypes as C

    from sgdnet_amd import _lib
    x = np.asfortranarray(rng.standard_normal((60, 4)))
    y1 = np.ascontiguousarray(x[:, 0] + rng.standard_normal(60))
    with pytest.raises(ValueError, match="must not be one-dimensional"):
        sa.cv_wmcovariance_fits(x, y1, np.arange(60) % 3, 0.5, [0.1, 0.01])
    ctl = _lib.Control()
    ctl.family, ctl.intercept, ctl.standardize, ctl.max_iter, ctl.tol, ctl.n_lambda, ctl.n_classes = 3, 1, 1, 100, 1e-7, 2, 1
    ctl.mode = _lib.MODE_WMCOVARIANCE
    out = [np.zeros(3 * 2), np.zeros(3 * 2 * 4), np.zeros(3 * 2), np.zeros(3 * 2), np.zeros(3), np.zeros(3)]
    res = _lib.CvMcovResult(*[_lib.dptr(a) for a in out])
    f32, alphas, lam = np.ascontiguousarray(np.arange(60) % 3, dtype=np.int32), np.array([0.5]), np.array([[0.1, 0.01]])
    L = sa.load()
    rc = L.sgdnet_cv_wmcovariance_dense(_lib.dptr(x), 60, 4, _lib.dptr(y1), f32.ctypes.data_as(C.POINTER(C.c_int32)), 3, 0, C.byref(ctl), 1,
                                        _lib.dptr(alphas), _lib.dptr(lam), C.byref(res))
    assert rc == -5 and L.sgdnet_last_error().decode().startswith("mode = wmcovariance needs at least two responses")
    # ... and the narrow CV refuses what it always refused, by its own name
    x196 = rng.standard_normal((30, 196))
    refused(sa.cv_mcovariance_fits, -5, "mode = mcovariance needs no more features than sgdnet_mcovariance_max_features(n_classes)", x196,
            x196[:, :2], np.arange(30) % 3)
    # the refusing calls left the device usable
    y = x[:, :2] + rng.standard_normal((60, 2))
    fits = sa.cv_wmcovariance_fits(x, y, np.arange(60) % 3, 0.5, [0.1, 0.01])
    assert len(fits) == 3 and all((f.return_codes == 0).all() for f in fits)
