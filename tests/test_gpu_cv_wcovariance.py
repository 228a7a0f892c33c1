"""Cross-validation in wide covariance mode: every fold fit of every alpha from ONE native call (sa.cv_wcovariance_fits ->
sgdnet_cv_wcovariance_*, sgdnet_amd/csrc/covariance.hip: wcovariance_cv_run) and cv_sgdnet_wcovariance(fold_fits="batched").

Fold fit (alpha, fold j) is BY DEFINITION sa.sgdnet_wcovariance(x[T], y[T], alpha=alpha, lambda_=lambda) for the training set
T of fold j.  The primary check is independent of any solver: the optimality conditions of that problem on x[T], y[T]
(sa.kkt) within the project's bound, for every job and every lambda, none dropped.  The second check is the separate fit
itself, to the project's figure for "the same optimum reached twice", wherever the optimum is unique: every training set
has more rows than features, or the mix is below 1.  Inputs, shapes and tolerances: tests/cv_wcovariance_reference.py."""
import numpy as np
import pytest
import scipy.sparse as sp

import cv_wcovariance_reference as cr
import test_gpu_covariance as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sa():
    import torch  # noqa: F401
    import sgdnet_amd
    if sgdnet_amd.load().sgdnet_device_count() < 1:
        pytest.fail("GPU tests need a HIP device; the backend has no CPU fallback")
    return sgdnet_amd


def assert_same_fit(got, ref, y_mean, what):
    """tests/test_gpu_cv_covariance.py: assert_same_fit (a0 relative to the larger of max|a0| and |mean_T(y)|)"""
    b = np.abs(got.beta - ref.beta).max() / np.abs(ref.beta).max()
    d = np.abs(got.dev_ratio - ref.dev_ratio).max() / np.abs(ref.dev_ratio).max()
    a = np.abs(got.a0 - ref.a0).max() / max(np.abs(ref.a0).max(), abs(y_mean))
    print(what, "vs the other fit: beta %.3g dev_ratio %.3g a0 %.3g" % (b, d, a))
    assert b <= cr.SAME_OPTIMUM and d <= cr.SAME_OPTIMUM and a <= cr.SAME_OPTIMUM, (what, b, d, a)
    assert got.nobs == ref.nobs and abs(got.nulldev - ref.nulldev) <= cr.SAME_OPTIMUM * ref.nulldev


def same_bytes(f, g):
    return all(getattr(f, name).tobytes() == getattr(g, name).tobytes() for name in ("beta", "a0", "dev_ratio", "return_codes")) and \
        f.npasses == g.npasses and f.nulldev == g.nulldev


def check_jobs(sa, x, y, foldid, mixes, train_on, standardize=True, intercept=True, compare=True, nlambda=6, lambda_min_ratio=1e-2, path=None):
    """one batched call over `mixes`; KKT on x[T], y[T] for every job and lambda, and the separate fit of every job whose
    optimum is unique.  path(mix) -> (nlambda, lambda_min_ratio) where the mixes have paths of their own"""
    opts = dict(standardize=standardize, intercept=intercept, **cr.TIGHT)
    lam = [cr.lambdas(x, y, m, standardize, *(path(m) if path else (nlambda, lambda_min_ratio))) for m in mixes]
    # one call takes one path length: a shorter path repeats its last lambda (user lambdas need not be monotone)
    longest = max(l.size for l in lam)
    lam = [np.concatenate([l, np.repeat(l[-1], longest - l.size)]) for l in lam]
    return check_lambdas(sa, x, y, foldid, mixes, lam, train_on, opts, compare)


def check_lambdas(sa, x, y, foldid, mixes, lam, train_on, opts, compare):
    standardize, intercept = opts["standardize"], opts["intercept"]
    fits = sa.cv_wcovariance_fits(x, y, foldid, mixes, lam, train_on=train_on, **opts)
    sets = cr.training_sets(foldid, train_on)
    assert len(fits) == len(mixes) * len(sets)
    for a, m in enumerate(mixes):
        for j, T in enumerate(sets):
            fit, xT, yT = fits[a * len(sets) + j], x[T], y[T]
            what = (x.shape, sp.issparse(x), m, train_on, standardize, intercept, j)
            assert (fit.return_codes == 0).all() and fit.draws_used == 0 and fit.alpha == m and fit.npasses > 0, (what, fit.return_codes)
            assert np.array_equal(fit.lambda_, lam[a]) and np.isfinite(fit.dev_ratio).all() and fit.nobs == T.sum()
            tc.assert_optimal(sa.kkt(fit, xT, yT, standardize=standardize, intercept=intercept), fit.lambda_, what)     # no job, no lambda dropped
            if compare and (T.sum() > x.shape[1] or m < 1.0):
                ref = sa.sgdnet_wcovariance(xT, yT, alpha=m, lambda_=lam[a], **opts)
                assert_same_fit(fit, ref, yT.mean(), what)
                assert (ref.return_codes == 0).all()
    return fits


# ---- 1. the envelope ----

# (the feature limit is a dense case: cv_wcovariance_reference.SHAPES)
ENVELOPE = [(shape, sparse, train_on) for shape in cr.SHAPES for sparse in (False, True) for train_on in ("fold", "rest")
            if not (sparse and shape[1] is None)]


@pytest.mark.parametrize("shape,sparse,train_on", ENVELOPE)
def test_every_fold_fit_is_optimal_and_the_separate_fit(sa, shape, sparse, train_on):
    n, p, G = shape[0], shape[1] or sa.wcovariance_max_features(), shape[2]
    x, y = cr.problem(n, p, sparse)
    mixes = cr.MIXES
    if shape[1] is None:
        mixes = [0.5]
    elif p == 1537:
        # one mix per case, chosen so that the four cases of this shape see all three
        mixes = [mixes[(2 * sparse + (train_on == "rest") + 1) % 3]]
    check_jobs(sa, x, y, cr.equal_folds(n, G), mixes, train_on, path=lambda m: cr.path_of(shape[1], m))


@pytest.mark.parametrize("train_on", ["fold", "rest"])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", [(195, 15, 3), (600, 198, 3)])
def test_same_optimum_as_the_narrow_cv(sa, shape, sparse, train_on):
    n, p, G = shape
    x, y = cr.problem(n, p, sparse, seed=8)
    foldid = cr.equal_folds(n, G, seed=8)
    lam = [cr.lambdas(x, y, m, True, 6, 1e-2) for m in cr.MIXES]
    wide = sa.cv_wcovariance_fits(x, y, foldid, cr.MIXES, lam, train_on=train_on, **cr.TIGHT)
    narrow = sa.cv_covariance_fits(x, y, foldid, cr.MIXES, lam, train_on=train_on, **cr.TIGHT)
    assert len(wide) == len(narrow) == 3 * G
    sets = cr.training_sets(foldid, train_on)
    for job, (w, c) in enumerate(zip(wide, narrow)):
        assert (w.return_codes == 0).all() and (c.return_codes == 0).all()
        assert_same_fit(w, c, y[sets[job % G]].mean(), (shape, sparse, train_on, job))


@pytest.mark.parametrize("train_on", ["fold", "rest"])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", [(195, 15, 3), (630, 199, 3)])
def test_intercept_and_standardize_combinations(sa, shape, sparse, train_on):
    n, p, G = shape
    x, y = cr.problem(n, p, sparse, seed=1)
    for intercept, standardize in ((True, False), (False, True), (False, False)):     # (True, True) is the test above
        check_jobs(sa, x, y, cr.equal_folds(n, G, seed=1), cr.MIXES, train_on, standardize=standardize, intercept=intercept)


# ---- 2. awkward folds at p = 199 (KKT only) ----

@pytest.mark.parametrize("sparse", [False, True])
def test_folds_cut_along_a_sorted_column(sa, sparse):
    x, y = cr.problem(630, 199, sparse, seed=2)
    for train_on in ("fold", "rest"):
        check_jobs(sa, x, y, cr.sorted_folds(x, 3), [0.5, 1.0], train_on, compare=False)


@pytest.mark.parametrize("sparse", [False, True])
def test_unequal_groups_a_group_of_one_and_labels_that_are_not_1_to_G(sa, sparse):
    x, y = cr.problem(630, 199, sparse, seed=3)
    foldid = cr.unequal_folds(630)
    assert sorted(np.bincount(foldid)[[10, 20, 30, 40]]) == [1, 209, 210, 210]
    check_jobs(sa, x, y, foldid, [0.5, 1.0], "rest", compare=False)      # (train_on="fold" cannot fit a single row's variance)


@pytest.mark.parametrize("sparse", [False, True])
def test_large_mean_column(sa, sparse):
    """a column of mean 1e6 and sd 1: on the path of tests/test_gpu_cv_covariance.py::test_large_mean_column (lambda_min_ratio =
    0.05) and for its reason -- a0 is about -7e5, one unit in its last place is 1.2e-10, and KKT_BOUND * lambda has to stay above
    what an f64 a0 can express"""
    x, y = cr.large_mean_problem(630, 199, sparse)
    for train_on in ("fold", "rest"):
        check_jobs(sa, x, y, cr.equal_folds(630, 3, seed=5), [0.5, 1.0], train_on, compare=False, **cr.LARGE_MEAN_PATH)


# ---- 3. more jobs than compute units ----

def test_more_jobs_than_compute_units(sa):
    n, p, G = cr.MANY_JOBS
    x, y = cr.problem(n, p, False, seed=4)
    fits = check_jobs(sa, x, y, np.arange(n), cr.MIXES, "rest")          # leave-one-out: every job optimal and its separate fit
    assert len(fits) == 270 > 256


# ---- 4. independence and determinism ----

@pytest.mark.parametrize("sparse", [False, True])
def test_jobs_are_independent_and_repeatable(sa, sparse):
    n, p, G = 630, 199, 3
    x, y = cr.problem(n, p, sparse, seed=6)
    foldid = cr.equal_folds(n, G, seed=6)
    lam = np.geomspace(1.0, 0.01, 6)
    kw = dict(thresh=1e-9, maxit=100000)
    alone = sa.cv_wcovariance_fits(x, y, foldid, [0.5], [lam], **kw)
    among = sa.cv_wcovariance_fits(x, y, foldid, [0.2, 0.5, 1.0], [lam, lam, lam], **kw)
    again = sa.cv_wcovariance_fits(x, y, foldid, [0.2, 0.5, 1.0], [lam, lam, lam], **kw)
    for j in range(G):
        assert same_bytes(alone[j], among[G + j]) and alone[j].npasses > 0, j
    for f, g in zip(among, again):
        assert same_bytes(f, g)


@pytest.mark.parametrize("shape", [(630, 199, 3), (130, 1025, 2)])
def test_both_widths_give_the_same_bits(sa, shape):
    n, p, G = shape
    x, y = cr.problem(n, p, False, seed=7)
    foldid = cr.equal_folds(n, G, seed=7)
    lam = [cr.lambdas(x, y, m, True, *cr.path_of(p, 0.5)) for m in (0.5, 1.0)]
    kw = dict(train_on="rest", **cr.TIGHT)
    with sa.option("wcovariance_width", 256):
        narrow = sa.cv_wcovariance_fits(x, y, foldid, [0.5, 1.0], lam, **kw)
    with sa.option("wcovariance_width", 1024):
        wide = sa.cv_wcovariance_fits(x, y, foldid, [0.5, 1.0], lam, **kw)
    for f, g in zip(narrow, wide):
        assert same_bytes(f, g) and (f.return_codes == 0).all() and f.npasses > 0
    with sa.option("wcovariance_width", 512):                  # not a width the library has
        with pytest.raises(sa.SgdnetError) as e:
            sa.cv_wcovariance_fits(x, y, foldid, [0.5, 1.0], lam, **kw)
    assert e.value.code == -1


def test_max_iter_is_reported_per_job_and_lambda(sa):
    n, p, G = 630, 199, 3
    x, y = cr.problem(n, p, False, seed=2)
    lam = [cr.lambdas(x, y, m, True, 5, 1e-2) for m in (0.5, 1.0)]
    fits = sa.cv_wcovariance_fits(x, y, cr.equal_folds(n, G), [0.5, 1.0], lam, thresh=1e-14, maxit=2)
    assert len(fits) == 2 * G
    for fit in fits:
        # below lambda_max no two sweeps change the coefficients by less than 1e-14 of their size
        # (tests/test_gpu_wcovariance.py::test_max_iter_is_reported)
        assert fit.npasses <= 2 * 5 and (fit.return_codes[1:] == 1).all(), fit.return_codes


# ---- 5. cv_sgdnet_wcovariance ----

@pytest.mark.parametrize("train_on", ["fold", "rest"])
def test_cv_sgdnet_wcovariance_batched_is_the_separate_cv(sa, train_on):
    x, y = cr.problem(630, 199, False)
    state, cvs = [], []
    for fold_fits in ("separate", "batched"):
        rng = sa.RRng(3)
        cvs.append(sa.cv_sgdnet_wcovariance(x, y, alpha=[0.5, 1], nfolds=3, rng=rng, train_on=train_on, nlambda=8, lambda_min_ratio=1e-2,
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
    assert sep.fit.beta.tobytes() == bat.fit.beta.tobytes()


# ---- 6. refusals ----

def test_refusals_name_the_condition(sa):
    rng = np.random.default_rng(0)
    limit = sa.wcovariance_max_features()

    def refused(fits, code, needle, xx, yy, ff):
        with pytest.raises(sa.SgdnetError) as e:
            fits(xx, yy, ff, 0.5, [0.1, 0.01])
        assert e.value.code == code and needle in str(e.value), str(e.value)

    wide = rng.standard_normal((6, limit + 1))
    refused(sa.cv_wcovariance_fits, -5, "mode = wcovariance needs no more features than sgdnet_wcovariance_max_features()", wide, wide[:, 0],
            np.arange(6) % 3)
    refused(sa.cv_wcovariance_fits, -5, "mode = wcovariance needs no more features", sp.csc_matrix(wide), wide[:, 0], np.arange(6) % 3)
    # the byte budget: enough groups of one row at a p where x itself stays small (8 MB)
    p = 1000
    G = cr.groups_over_budget(p)
    big = rng.standard_normal((G, p))
    refused(sa.cv_wcovariance_fits, -5, "mode = wcovariance needs the moments and the scaled matrices of the groups within %d bytes" % cr.BUDGET_BYTES,
            big, big[:, 0], np.arange(G))
    # ... and the narrow CV refuses what it always refused, by its own name
    x199 = rng.standard_normal((30, 199))
    refused(sa.cv_covariance_fits, -5, "mode = covariance needs no more features", x199, x199[:, 0], np.arange(30) % 3)
